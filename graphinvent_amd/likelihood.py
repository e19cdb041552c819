"""
Log-likelihood of whole molecules under a model: how likely is this given molecule?

For molecule ``m`` with decoding-route rows ``k = 0 .. n_edges + 1`` (exactly the rows of
``routes.expand(merge=False)``), logits ``z_k = model(nodes_k, edges_k)`` and hot APD index ``a_k``::

    ll_m = sum_k ( z_k[a_k] - logsumexp(z_k) )

which is the log of the product, over the route, of the per-row probability that
``Analyzer.get_validation_likelihood`` (Analyzer.py:754-774) computes for a one-hot target.  One deviation from the
reference's arithmetic: the value is evaluated in log space with the row maximum subtracted, so it stays finite
where the reference's linear-space expression (``softmax``, product with the target, row sum, ``log``) underflows.

The reference has this number per subgraph row of a preprocessed file only, and its RL loop per molecule it has
just sampled; here it is available for any stored molecule: held-out NLL per molecule, the prior's or the agent's
likelihood of a set of actives, ranking a library.  The routes are expanded on the device (``csrc/gi_route.hip``)
WITHOUT their APD rows, whose only use would be a product with a softmax; the hot index of every row is all that is
kept of them.  The row and molecule kernels are in ``csrc/gi_loglik.hip``.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import lib as L
from . import routes as R
from .generator import _host_sync_allowed

ERROR_MESSAGES = {
    L.LL_ERR_HOT: "a hot index is outside [-1, W)",
    L.LL_ERR_MOL: "a row_mol entry is outside [-1, n_molecules)",
    L.LL_ERR_ORDER: "row_mol decreases (the rows of a molecule must be consecutive, molecules in ascending order)",
}


def _describe(bits: int) -> str:
    return "; ".join(msg for bit, msg in ERROR_MESSAGES.items() if bits & bit)


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _check_rows(logits: torch.Tensor, hot: torch.Tensor) -> torch.Tensor:
    if not (torch.is_tensor(logits) and torch.is_tensor(hot)):
        raise TypeError("logits and hot must be torch tensors on the GPU")
    if not (logits.is_cuda and hot.is_cuda):
        raise RuntimeError("logits and hot must be CUDA (ROCm) tensors: the likelihood kernels have no CPU fallback")
    if logits.device != hot.device:
        raise ValueError("logits and hot are on different devices")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[1] < 1:
        raise TypeError(f"logits must be fp32 [rows, W], W >= 1, got {logits.dtype} {tuple(logits.shape)}")
    if hot.dtype != torch.int32 or hot.dim() != 1 or hot.shape[0] != logits.shape[0] or not hot.is_contiguous():
        raise TypeError("hot must be a contiguous int32 tensor with one entry per row of logits")
    if logits.shape[0] and not (logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]):
        logits = logits.contiguous()
    return logits


def _row_forward(logits: torch.Tensor, hot: torch.Tensor, err: torch.Tensor):
    """gi_row_loglik on the current stream: (row_ll, row_lse), zero where the kernel writes nothing."""
    rows, W = logits.shape
    out = torch.zeros((2, rows), dtype=torch.float32, device=logits.device)
    if rows:
        with torch.cuda.device(logits.device):
            L.check(L.load().gi_row_loglik(logits.data_ptr(), logits.stride(0), rows, W, hot.data_ptr(),
                                           out[0].data_ptr(), out[1].data_ptr(), err.data_ptr(),
                                           _stream(logits.device)), "gi_row_loglik")
    return out[0], out[1]


def _row_backward(logits, hot, row_lse, g, err, row_mol=None, g_kind=None, n_add=0, n_conn=0):
    """gi_row_loglik_bwd on the current stream: d_logits [rows, W], contiguous.  ``g`` is per molecule when
    ``row_mol`` is given and per row otherwise."""
    rows, W = logits.shape
    d = torch.empty((rows, W), dtype=torch.float32, device=logits.device)
    if rows:
        g = g.to(torch.float32).contiguous()
        if g_kind is not None:
            g_kind = g_kind.to(torch.float32).contiguous()
        with torch.cuda.device(logits.device):
            L.check(L.load().gi_row_loglik_bwd(
                logits.data_ptr(), logits.stride(0), rows, W, hot.data_ptr(), row_lse.data_ptr(), g.data_ptr(),
                None if g_kind is None else g_kind.data_ptr(), None if row_mol is None else row_mol.data_ptr(),
                g.shape[0], n_add, n_conn, d.data_ptr(), W, err.data_ptr(), _stream(logits.device)),
                "gi_row_loglik_bwd")
    return d


def _mol_sum(row_ll, row_mol, hot, W, n_add, n_conn, mol_ll, mol_kind, err) -> None:
    """gi_mol_loglik_sum on the current stream: mol_ll (and mol_kind) += the rows of this call."""
    with torch.cuda.device(row_ll.device):
        L.check(L.load().gi_mol_loglik_sum(row_ll.data_ptr(), row_mol.data_ptr(), hot.data_ptr(), row_ll.shape[0],
                                           mol_ll.shape[0], W, n_add, n_conn, mol_ll.data_ptr(),
                                           None if mol_kind is None else mol_kind.data_ptr(), err.data_ptr(),
                                           _stream(row_ll.device)), "gi_mol_loglik_sum")


class _RowLogLik(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, hot, err):
        row_ll, row_lse = _row_forward(logits, hot, err)
        ctx.save_for_backward(logits, hot, row_lse, err)
        return row_ll

    @staticmethod
    def backward(ctx, g):
        logits, hot, row_lse, err = ctx.saved_tensors
        return _row_backward(logits, hot, row_lse, g, err), None, None


def row_log_likelihood(logits: torch.Tensor, hot: torch.Tensor, err: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``logits[r, hot[r]] - logsumexp(logits[r])`` for every row, fp32 ``[rows]``, differentiable in ``logits``.

    ``logits`` fp32 ``[rows, W]`` (any row pitch, any ``W >= 1``), ``hot`` int32 ``[rows]``, both on the GPU.  Each
    row is read once.  A row with ``hot == -1`` (a padding row) gives 0 and an exactly zero gradient row; a NaN logit
    gives NaN; a row whose hot logit is -inf gives -inf.  ``err`` (int32, one element, on the device): a ``hot``
    outside ``[-1, W)`` ORs ``lib.LL_ERR_HOT`` into it and the row gives 0 — nothing is indexed with such a value
    and nothing is read back here, so pass ``err`` to learn of it."""
    logits = _check_rows(logits, hot)
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=logits.device)
    elif not (err.is_cuda and err.dtype == torch.int32 and err.numel() >= 1 and err.is_contiguous()):
        raise TypeError("err must be a contiguous int32 tensor on the GPU")
    return _RowLogLik.apply(logits, hot, err)


class _ChunkLogLik(torch.autograd.Function):
    """One chunk of rows: row kernel, then the molecule sums accumulated IN PLACE into ``mol_ll`` (and ``mol_kind``),
    which are returned — the chunks of a call form a chain through them, so that the no-grad and the differentiable
    path add the same numbers in the same order."""

    @staticmethod
    def forward(ctx, logits, hot, row_mol, err, n_add, n_conn, mol_ll, mol_kind):
        row_ll, row_lse = _row_forward(logits, hot, err)
        _mol_sum(row_ll, row_mol, hot, logits.shape[1], n_add, n_conn, mol_ll, mol_kind, err)
        ctx.save_for_backward(logits, hot, row_mol, row_lse, err)
        ctx.kinds = (n_add, n_conn)
        if mol_kind is None:
            ctx.mark_dirty(mol_ll)
            return mol_ll
        ctx.mark_dirty(mol_ll, mol_kind)
        return mol_ll, mol_kind

    @staticmethod
    def backward(ctx, g_ll, g_kind=None):
        logits, hot, row_mol, row_lse, err = ctx.saved_tensors
        if g_ll is None:
            g_ll = torch.zeros(g_kind.shape[0], dtype=torch.float32, device=logits.device)
        d = _row_backward(logits, hot, row_lse, g_ll, err, row_mol, g_kind, *ctx.kinds)
        return d, None, None, None, None, None, g_ll, g_kind


def completion_hot(hot: torch.Tensor, row_mol: torch.Tensor, row_step: torch.Tensor, lengths: torch.Tensor,
                   given_actions: torch.Tensor) -> torch.Tensor:
    """``hot`` with -1 on the rows of the given part of every route.  Row ``k`` of a route is the state before the
    ``k``-th last build action (``k = 0`` the terminate), and molecule ``m`` has ``lengths[m] - 1 = n_edges + 1``
    build actions: with the first ``given_actions[m]`` of them given, the rows that stay are those with
    ``row_step <= n_edges + 1 - given_actions[m]``.  Torch ops on the tensors' device, no read-back."""
    m = row_mol.clamp(min=0).long()
    last = (lengths.to(torch.int32) - 1 - given_actions.to(torch.int32))[m]
    return torch.where((row_mol < 0) | (row_step > last), -1, hot).to(torch.int32)


class _Scored:
    """The expansion of a call and what its chunk loop needs."""

    def __init__(self, nodes, edges, dim_f_add, dim_f_conn, batch_rows, n_rows, invalid, given_actions=None):
        if invalid not in ("raise", "skip"):
            raise ValueError("invalid must be 'raise' or 'skip'")
        if int(batch_rows) < 1:
            raise ValueError("batch_rows must be >= 1")
        nodes, edges = R._check_inputs(nodes, edges)
        M, N, Fn = nodes.shape
        self.d = d = R._route_dims(M, N, Fn, edges.shape[3], dim_f_add, dim_f_conn)
        self.dev, self.M, self.W, self.invalid, self.batch_rows = nodes.device, M, d.apd_width, invalid, int(batch_rows)
        self.n_conn = N * d.Fe
        self.n_add = self.W - 1 - self.n_conn
        self.p = None
        self.given_bad = None
        if given_actions is not None:
            with _host_sync_allowed():                               # (set-up: a host sequence's upload)
                given_actions = torch.as_tensor(given_actions)
                if tuple(given_actions.shape) != (M,) or given_actions.dtype.is_floating_point:
                    raise ValueError(f"given_actions must be {M} integers, one per molecule")
                given_actions = given_actions.to(device=self.dev, dtype=torch.int32)
        if M == 0:
            return
        with torch.cuda.device(self.dev):
            planned = None
            self.expect = None if n_rows is None else int(n_rows)
            if n_rows is None:
                planned = R._plan(nodes, edges, d)
                with _host_sync_allowed():
                    head = planned[3].cpu().tolist()             # read-back: sizes the outputs
                if head[0] and invalid == "raise":
                    raise ValueError("invalid molecule(s) in the batch: " + R.describe_errors(head[0]))
                n_rows = head[1]
            self.p = p = R._enqueue(nodes, edges, d, False, int(n_rows), planned, _apds=False)
            cap = p.cap
            self.nodes = p.nodes[:cap * N * Fn].view(cap, N, Fn)
            self.edges = p.edges[:cap * N * N * d.Fe].view(cap, N, N, d.Fe)
            self.row_mol = p.row_mol[:cap]
            # the rows past the real ones (an n_rows larger than the molecules need, skipped molecules) are padding
            self.hot = torch.where(self.row_mol < 0, -1, p.hot).to(torch.int32)
            if given_actions is not None:
                self.hot = completion_hot(self.hot, self.row_mol, p.row_step[:cap], p.lengths, given_actions)
                self.given_bad = (((given_actions < 0) | (given_actions > p.lengths - 1)) & (p.mol_err == 0)).any()
            self.err = torch.zeros(1, dtype=torch.int32, device=self.dev)

    def chunks(self):
        for a in range(0, self.p.cap, self.batch_rows):
            b = min(a + self.batch_rows, self.p.cap)
            yield self.nodes[a:b], self.edges[a:b], self.hot[a:b], self.row_mol[a:b]

    def finish(self, model, mol_ll, mol_kind):
        """The call's read-back (the expansion's error bits and row count, the kernels' error word, a sync-free
        model's sticky bounds error), after the loop; NaN for the molecules the planner refused."""
        p = self.p
        with _host_sync_allowed():
            counts = p.counts.cpu().tolist()
            bits = int(self.err.item())
            given_bad = self.given_bad is not None and bool(self.given_bad.item())
            if getattr(model, "sync_free", False) and hasattr(model, "last_bounded_error"):
                model.last_bounded_error()
        err, total = int(counts[0]), int(counts[1])
        if err and self.invalid == "raise":
            raise ValueError("invalid molecule(s) in the batch: " + R.describe_errors(err))
        if total > p.cap or (self.expect is not None and not err and total != self.expect):
            raise ValueError(f"the molecules expand to {total} rows, not the {p.cap} the call was sized for "
                             "(n_rows must be route_lengths(nodes, edges).sum())")
        if given_bad:
            raise ValueError("given_actions: a value is outside [0, n_edges + 1] of its molecule")
        if bits:
            raise RuntimeError("graphinvent_amd likelihood: " + _describe(bits))
        if self.invalid == "raise":
            return mol_ll, mol_kind, None
        bad = p.mol_err != 0
        nan = float("nan")
        mol_ll = torch.where(bad, nan, mol_ll)
        if mol_kind is not None:
            mol_kind = torch.where(bad[:, None], nan, mol_kind)
        return mol_ll, mol_kind, p.mol_err


def _result(ll, kind, mol_err, by_kind, invalid):
    out = (ll,) + ((kind,) if by_kind else ()) + ((mol_err,) if invalid == "skip" else ())
    return out[0] if len(out) == 1 else out


def molecule_log_likelihood(model, nodes: torch.Tensor, edges: torch.Tensor, dim_f_add: Sequence[int],
                            dim_f_conn: Sequence[int], *, batch_rows: int = 1000, by_kind: bool = False,
                            n_rows: Optional[int] = None, invalid: str = "raise", given_actions=None):
    """``ll_m`` (module docstring) of ``M`` whole molecules under ``model``: fp32 ``[M]`` on the molecules' device.

    ``nodes`` / ``edges``: int8 device molecules ``[M, N, Fn]`` / ``[M, N, N, Fe]`` under ``routes.expand``'s
    contract (nodes in a BFS / DFS order, zero padded); run ``routes.reorder`` first for any other node order — the
    value is the likelihood of THAT decoding route, not a marginal over node orders.  The routes are planned and
    expanded without merge and without allocating or writing the APD rows; ``model`` then runs on consecutive
    chunks of ``batch_rows`` rows, irrespective of molecule boundaries (a route cut by a chunk boundary is
    continued by the next chunk; the sum of a molecule is one sequential fp32 sum in route order whatever
    ``batch_rows`` is).

    ``by_kind=True`` appends fp32 ``[M, 3]``: the sum split by action kind — add (``a_k < N A``), connect
    (``a_k < N A + N Fe``), terminate (the last index).

    Differentiable with respect to the model's parameters when grad is enabled.  Every chunk's tape is then kept
    until the backward (about 0.6 GB per 1000 rows at the headline model): for maximum-likelihood fine-tuning on a
    large set use ``weighted_log_likelihood_backward``, which streams.

    Host synchronisation: ``n_rows = routes.route_lengths(nodes, edges).sum()``, when the caller has it from the
    host copies, saves the read-back that sizes the expansion.  Under ``torch.no_grad`` with ``model.sync_free =
    True`` and ``n_rows`` given the chunk loop has no host synchronisation at all; the call's one read-back (error
    bits, row count) comes after the loop.

    ``invalid="raise"``: a molecule that violates the contract raises ``ValueError`` naming the rule.  ``"skip"``:
    such molecules give NaN and the per-molecule error bits (int32 ``[M]``, ``lib.ROUTE_ERR_*``) are appended to
    the result, as ``routes.reorder`` does.  ``M == 0`` returns empty tensors; CPU tensors raise ``RuntimeError``.

    ``given_actions`` (int32 ``[M]`` device tensor, or a sequence; default None = 0 everywhere, bit-identical):
    the likelihood of a COMPLETION.  The first ``given_actions[m]`` build actions of molecule ``m``'s route (a
    molecule has ``n_edges + 1`` of them: its first atom, then one per bond) are taken as given — e.g.
    ``SeedBank.n_actions`` of the seed a generated molecule was grown from — and the sum runs over the rest, the
    terminate included: the rows with ``row_step <= n_edges + 1 - given_actions[m]``.  The other rows still pass
    through the model but enter with ``hot = -1``, which the kernels turn into exact zeros, forward and backward;
    ``by_kind`` follows the same mask.  A value outside ``[0, n_edges + 1]`` raises ``ValueError`` (with the call's
    read-back, after the loop).  Because the route fixes ONE order of a node's ring-closing bonds, this value equals
    the completion likelihood the generator recorded for a sampled molecule only when the sampled order was the
    route's.
    """
    s = _Scored(nodes, edges, dim_f_add, dim_f_conn, batch_rows, n_rows, invalid, given_actions)
    mol_ll = torch.zeros(s.M, dtype=torch.float32, device=s.dev)
    mol_kind = torch.zeros((s.M, 3), dtype=torch.float32, device=s.dev) if by_kind else None
    if s.M == 0:
        return _result(mol_ll, mol_kind, torch.zeros(0, dtype=torch.int32, device=s.dev), by_kind, invalid)
    with torch.cuda.device(s.dev):
        for cn, ce, hot, row_mol in s.chunks():
            logits = _check_rows(model(cn, ce), hot)
            if logits.shape[1] != s.W:
                raise ValueError(f"the model returns rows of {logits.shape[1]} logits; dim_f_add / dim_f_conn give "
                                 f"{s.W}")
            out = _ChunkLogLik.apply(logits, hot, row_mol, s.err, s.n_add, s.n_conn, mol_ll, mol_kind)
            mol_ll, mol_kind = out if by_kind else (out, None)
        return _result(*s.finish(model, mol_ll, mol_kind), by_kind, invalid)


def weighted_log_likelihood_backward(model, nodes: torch.Tensor, edges: torch.Tensor, dim_f_add: Sequence[int],
                                     dim_f_conn: Sequence[int], weights: torch.Tensor, *, batch_rows: int = 1000,
                                     n_rows: Optional[int] = None, invalid: str = "raise", given_actions=None):
    """Accumulates the gradients of ``sum_m weights[m] * ll_m`` with respect to the model's parameters into their
    ``.grad`` and returns the ``ll`` values (detached; with ``invalid="skip"`` also the error bits), for the
    arguments of ``molecule_log_likelihood``.

    One forward and one backward per chunk of ``batch_rows`` rows: only one chunk's tape is alive at a time,
    whatever the size of the set.  This is exact, not an approximation: once the weights are known the objective is
    linear in the row terms, so the gradient of the whole is the sum of the chunks' gradients, each taken with
    ``d objective / d row_ll[r] = weights[row_mol[r]]``.  ``weights`` (``[M]``, on the molecules' device) is a
    constant here; a molecule that ``invalid="skip"`` refuses has no rows and contributes nothing.
    ``given_actions``: as in ``molecule_log_likelihood`` — the given rows contribute neither value nor gradient."""
    s = _Scored(nodes, edges, dim_f_add, dim_f_conn, batch_rows, n_rows, invalid, given_actions)
    if not torch.is_tensor(weights) or tuple(weights.shape) != (s.M,):
        raise ValueError(f"weights must be a tensor of {s.M} entries, one per molecule")
    if s.M and weights.device != s.dev:
        raise RuntimeError("weights must be on the molecules' device: the likelihood kernels have no CPU fallback")
    mol_ll = torch.zeros(s.M, dtype=torch.float32, device=s.dev)
    if s.M == 0:
        return _result(mol_ll, None, torch.zeros(0, dtype=torch.int32, device=s.dev), False, invalid)
    w = weights.detach().to(torch.float32).contiguous()
    with torch.cuda.device(s.dev):
        for cn, ce, hot, row_mol in s.chunks():
            with torch.enable_grad():
                logits = model(cn, ce)
            with torch.no_grad():
                z = _check_rows(logits.detach(), hot)
                if z.shape[1] != s.W:
                    raise ValueError(f"the model returns rows of {z.shape[1]} logits; dim_f_add / dim_f_conn give "
                                     f"{s.W}")
                row_ll, row_lse = _row_forward(z, hot, s.err)
                _mol_sum(row_ll, row_mol, hot, s.W, s.n_add, s.n_conn, mol_ll, None, s.err)
                d = _row_backward(z, hot, row_lse, w, s.err, row_mol)
            if logits.requires_grad:
                logits.backward(d)
        return _result(*s.finish(model, mol_ll, None), False, invalid)
