"""
Generation loop on the device: ``GraphGenerator.build_graphs`` (GraphGenerator.py:99-161) as rounds of

    forward  ->  ``gi_sample_actions`` (sampler.sample_actions_raw)  ->  ``gi_grow_graphs`` (grow_step)

with no read-back inside a round.  ``gi_grow_graphs`` is the reference's bookkeeping after the draw —
``properly_terminated``, ``copy_terminated_graphs``, ``apply_actions``, ``reset_graphs`` and the dummy graph's restore
(:126-157, 211-465) — taken straight from the sampler's per-graph action / likelihood / flags, in place on the
generator's own tensors.  Its counters (graphs generated, round, target, error) live on the device, are mirrored into
mapped host memory, and freeze the step once the target is reached or an error was flagged: rounds enqueued after
that change nothing, so the host only has to look every few rounds.

``build_graphs(gen, constants.dim_f_add, constants.dim_f_conn)`` is the drop-in for ``gen.build_graphs()``; after it
every tensor the reference's loop writes (``generated_*``, ``properly_terminated``, ``nodes``, ``edges``,
``n_nodes``, ``likelihoods``) holds what the reference leaves for the same draws.

``build_graphs_rl(gen, constants.dim_f_add, constants.dim_f_conn)`` is the same for ``GraphGeneratorRL.build_graphs``
(GraphGeneratorRL.py:109-172), with gradients: both models run with grad, ``sample_actions_rl``'s autograd Function
draws, and ``gi_grow_graphs_rl`` carries both likelihood streams and records each generated row's trajectory (source
graph, first and last round).  The generated likelihood rows are then rebuilt from the stacked per-round likelihoods
by an autograd Function (``gi_grow_traj_gather`` forward, ``gi_grow_traj_scatter`` backward), so that
``Workflow.compute_loss_component`` differentiates through every applied round into both models.

Seeded generation (scaffold decoration, fragment growing): ``build_graphs(..., seeds=SeedBank(...))`` and
``build_graphs_rl(..., seeds=...)`` start every graph from a molecule of the bank instead of from the empty graph, and
restart it from the next one when it is written out (``gi_grow_seed_init``, ``gi_grow_graphs_seeded``,
``gi_grow_graphs_rl_seeded``): still no read-back inside a round, in the blocking, sync-free and captured modes alike.
``gen.generated_seed`` then names the seed behind every generated row, and the generated likelihood rows are those of
the COMPLETION given the seed (``likelihood.molecule_log_likelihood(..., given_actions=bank.n_actions[...])`` scores
the same quantity for stored molecules).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as L
from . import routes as R
from .sampler import ActionConstraint, _add_dims, _MaskActions, _SampleRL, mask_actions_raw, sample_actions_raw

#: the generator tensors the step reads and writes, in gi_grow_desc's order, with their dtypes
_STATE_TENSORS = (("nodes", torch.float32), ("edges", torch.float32), ("n_nodes", torch.int8),
                  ("likelihoods", torch.float32), ("generated_nodes", torch.float32),
                  ("generated_edges", torch.float32), ("generated_n_nodes", torch.int8),
                  ("generated_likelihoods", torch.float32), ("properly_terminated", torch.int8))


def new_state(batch_size: int, target: int, device, rl: bool = False, seeded: bool = False) -> torch.Tensor:
    """The step's device state: int32 [GI_GROW_STATE_WORDS + B] (``rl``: + 2 B, ``gi_grow_rl_state_words``;
    ``seeded``, with or without ``rl``: + 3 B, ``gi_grow_seeded_state_words``), zero with ``state[2] = target``."""
    words = L.GROW_STATE_WORDS + (3 if seeded else 2 if rl else 1) * batch_size
    state = torch.zeros(words, dtype=torch.int32, device=device)
    state.narrow(0, 2, 1).fill_(int(target))          # a fill launch: no host -> device copy
    return state


def _validate(t: dict, dim_f_add: Sequence[int], dim_f_conn: Sequence[int]):
    """What gi_grow_desc needs of the generator tensors ``t`` (dtypes, layout, shapes, one CUDA device); returns
    ``(B, N, Fn, Fe, L, C)``, the add's sub-dimensions and its node-feature groups."""
    nodes, edges = t["nodes"], t["edges"]
    for name, dtype in _STATE_TENSORS:
        x = t[name]
        if x.dtype != dtype:
            raise TypeError(f"{name} must be {dtype} (the reference's dtype), got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous: the step writes it in place")
    if nodes.dim() != 3 or edges.dim() != 4:
        raise ValueError("nodes must be [B, N, Fn] and edges [B, N, N, Fe]")
    B, N, Fn = nodes.shape
    Fe = edges.shape[3]
    sub, _ = _add_dims(edges, dim_f_add, dim_f_conn)
    groups = sub[:-1]
    if sub[-1] != Fe or not groups or len(groups) > L.GROW_MAX_GROUPS or sum(groups) != Fn:
        raise ValueError(f"dim_f_add {list(dim_f_add)} does not match nodes {tuple(nodes.shape)} / edges "
                         f"{tuple(edges.shape)}: the add's node-feature groups must tile Fn, bond type last")
    Lc = t["likelihoods"].shape[1] if t["likelihoods"].dim() == 2 else -1
    Cg = t["generated_nodes"].shape[0]
    want = {"edges": (B, N, N, Fe), "n_nodes": (B,), "likelihoods": (B, Lc),
            "generated_nodes": (Cg, N, Fn), "generated_edges": (Cg, N, N, Fe), "generated_n_nodes": (Cg,),
            "generated_likelihoods": (Cg, Lc), "properly_terminated": (Cg,)}
    for name, shape in want.items():
        if tuple(t[name].shape) != shape:
            raise ValueError(f"{name} has shape {tuple(t[name].shape)}, expected {shape}")
    if Lc < 1 or Cg < 1:
        raise ValueError("the likelihood and generated buffers must not be empty")
    for name, _ in _STATE_TENSORS:
        x = t[name]
        if not x.is_cuda:
            raise RuntimeError(f"grow_step needs CUDA (ROCm) tensors ({name} is on {x.device}): the MI355X HIP "
                               "path has no CPU fallback")
        if x.device != nodes.device:
            raise ValueError(f"{name} is on {x.device}, nodes on {nodes.device}")
    return (B, N, Fn, Fe, Lc, Cg), sub, groups


class SeedBank:
    """A bank of ``S >= 1`` seed molecules (scaffolds, fragments) for seeded generation: int8 device molecules
    ``nodes [S, N, Fn]`` / ``edges [S, N, N, Fe]`` in the loader's format, validated once on the device with
    ``routes.check`` (0 / 1 entries, one-hot feature groups, symmetric edges with one bond type per pair, zero-padded
    prefix, every node i > 0 bonded to a node of lower index — which implies a connected molecule); an all-zero
    molecule is accepted as the empty seed.  ``reorder="bfs"`` / ``"dfs"`` runs ``routes.reorder`` first, so seeds in
    any node order are accepted.  ONE read-back, here; a violated rule raises ``ValueError`` naming it.

    ``n_nodes`` (int8 ``[S]``) and ``n_actions`` (int32 ``[S]``: the build actions a seed stands for, ``n_edges + 1``,
    0 for the empty seed — the ``given_actions`` of ``likelihood.molecule_log_likelihood``) are on the device.
    The generation loops take the seeds round-robin in bank order: shuffle the molecules before building the bank
    to randomise."""

    def __init__(self, nodes: torch.Tensor, edges: torch.Tensor, dim_f_add: Sequence[int],
                 dim_f_conn: Sequence[int], *, reorder: Optional[str] = None):
        if reorder not in (None, "bfs", "dfs"):
            raise ValueError("reorder must be None, 'bfs' or 'dfs'")
        nodes, edges = R._check_inputs(nodes, edges)
        if nodes.shape[0] < 1:
            raise ValueError("a seed bank needs at least one molecule (the all-zero molecule is the empty seed)")
        with torch.cuda.device(nodes.device):
            empty = ~((nodes != 0).flatten(1).any(1) | (edges != 0).flatten(1).any(1))
            bits = torch.zeros(nodes.shape[0], dtype=torch.int32, device=nodes.device)
            if reorder is not None:
                nodes, edges, bits = R.reorder(nodes, edges, route=reorder, invalid="skip")
            disconnected = (bits & L.ROUTE_ERR_CONNECT) != 0              # (reorder's meaning of the bit)
            bits = (bits & ~L.ROUTE_ERR_CONNECT) | R.check(nodes, edges, dim_f_add, dim_f_conn)
            bits = torch.where(empty, bits & ~L.ROUTE_ERR_EMPTY, bits)
            n_nodes = (nodes != 0).flatten(2).any(2).sum(1)
            n_edges = (edges != 0).flatten(1).sum(1) // 2
            with _host_sync_allowed():
                flags = torch.stack((bits, disconnected.to(torch.int32))).cpu().numpy()      # the read-back
        bad = flags[0] != 0
        if bad.any() or flags[1].any():
            what = R.describe_errors(int(np.bitwise_or.reduce(flags[0])))
            if flags[1].any():
                what = "; ".join(filter(None, [what, "a molecule is not connected"]))
            first = int((bad | (flags[1] != 0)).argmax())
            raise ValueError(f"invalid seed(s) in the bank (first: seed {first}): {what}")
        self.nodes, self.edges = nodes, edges
        self.n_nodes = n_nodes.to(torch.int8)
        self.n_actions = torch.where(empty, 0, n_edges + 1).to(torch.int32)
        self.device = nodes.device

    def __len__(self) -> int:
        return self.nodes.shape[0]

    def desc(self, N: int, Fn: int, Fe: int, device, gen_seed: Optional[torch.Tensor]) -> "L.GrowSeedDesc":
        """gi_grow_seed_desc for generator tensors of the given dims (checked against the bank's)."""
        S, bN, bFn = self.nodes.shape
        bFe = self.edges.shape[3]
        if (bN, bFn, bFe) != (N, Fn, Fe):
            raise ValueError(f"the seed bank has N, Fn, Fe = {(bN, bFn, bFe)}, the generator's tensors {(N, Fn, Fe)}")
        if self.device != device:
            raise ValueError(f"the seed bank is on {self.device}, the generator's tensors on {device}")
        d = L.GrowSeedDesc()
        d.nodes, d.edges, d.n_nodes = self.nodes.data_ptr(), self.edges.data_ptr(), self.n_nodes.data_ptr()
        d.gen_seed = gen_seed.data_ptr() if gen_seed is not None else None
        d.S = S
        return d


def _check_gen_seed(gen_seed: Optional[torch.Tensor], Cg: int, device) -> None:
    if gen_seed is not None and (gen_seed.dtype != torch.int32 or tuple(gen_seed.shape) != (Cg,) or
                                 not gen_seed.is_contiguous() or gen_seed.device != device):
        raise ValueError(f"generated_seed must be a contiguous int32 [{Cg}] tensor on {device}")


class _Masker:
    """The mask step of a constrained loop: ``constraint`` checked against the generator tensors ``t`` once, the running
    figures (``stats``) allocated before any round — and so before a capture — and kept on the device.  ``raw`` /
    ``rl`` enqueue one gi_action_mask launch on the graphs' current state and one small launch that adds the round to
    the figures unless the growth ``state`` shows a frozen round (graph 0, the dummy, is left out of them)."""

    def __init__(self, constraint, t: dict, state: torch.Tensor):
        if not isinstance(constraint, ActionConstraint):
            raise TypeError(f"constraint must be a sampler.ActionConstraint, got {type(constraint).__name__}")
        nodes, edges = t["nodes"], t["edges"]
        c = constraint
        if nodes.dim() != 3 or edges.dim() != 4 or tuple(nodes.shape[1:]) != (c.N, c.Fn) or \
                tuple(edges.shape[1:]) != (c.N, c.N, c.Fe):
            raise ValueError(f"the constraint was built for N, Fn, Fe = {(c.N, c.Fn, c.Fe)}, the generator's tensors "
                             f"are nodes {tuple(nodes.shape)} / edges {tuple(edges.shape)}")
        if nodes.device != c.device:
            raise ValueError(f"the constraint's rules are on {c.device}, the generator's tensors on {nodes.device}")
        self.c, self.t, self.state, self.device = c, t, state, nodes.device
        self.counts = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.mass = torch.zeros(1, dtype=torch.float32, device=self.device)

    @property
    def stats(self) -> dict:
        return {"rounds": self.counts[0], "graph_rounds_masked": self.counts[1], "mass_removed": self.mass[0]}

    def _account(self, removed: torch.Tensor) -> None:
        B = removed.shape[0]
        with torch.cuda.device(self.device):
            L.check(L.load().gi_action_mask_stats(B - 1, removed.data_ptr() + 4, self.state.data_ptr(),
                                                  self.counts.data_ptr(), self.mass.data_ptr(),
                                                  torch.cuda.current_stream(self.device).cuda_stream),
                    "gi_action_mask_stats")

    def raw(self, logits: torch.Tensor, account: bool = True) -> torch.Tensor:
        t = self.t
        masked, _, _, _, _, removed = mask_actions_raw(logits, t["n_nodes"], t["nodes"], t["edges"], self.c,
                                                       bits=False, removed=True)
        if account:
            self._account(removed)
        return masked

    def rl(self, agent_logits: torch.Tensor, prior_logits: torch.Tensor):
        t = self.t
        masked_a, masked_p, _, _, _, removed = _MaskActions.apply(agent_logits, prior_logits, t["n_nodes"], t["nodes"],
                                                                 t["edges"], self.c, False, False, True)
        self._account(removed)
        return masked_a, masked_p


class _Grower:
    """Validated gi_grow_desc of one set of generator tensors; ``step`` enqueues one round.  With ``seeds`` (a
    SeedBank) the rounds are gi_grow_graphs_seeded's, ``seed_init`` enqueues the first fill and ``gen_seed`` (int32
    [C], optional) receives the seed of every generated row."""

    def __init__(self, t: dict, dim_f_add: Sequence[int], dim_f_conn: Sequence[int], state: torch.Tensor,
                 host_state: Optional[int] = None, seeds: Optional[SeedBank] = None,
                 gen_seed: Optional[torch.Tensor] = None):
        (B, N, Fn, Fe, Lc, Cg), sub, groups = _validate(t, dim_f_add, dim_f_conn)
        nodes = t["nodes"]
        if state.dtype != torch.int32 or state.device != nodes.device or not state.is_contiguous() or \
                state.numel() < L.GROW_STATE_WORDS + B:
            raise ValueError("state must be a contiguous int32 tensor of GI_GROW_STATE_WORDS + B words on the "
                             "tensors' device (generator.new_state)")
        self.seeds, self.gen_seed, self.seed_desc = seeds, gen_seed, None
        if seeds is not None:
            if not isinstance(seeds, SeedBank):
                raise TypeError("seeds must be a generator.SeedBank")
            _check_gen_seed(gen_seed, Cg, nodes.device)
            self.seed_desc = seeds.desc(N, Fn, Fe, nodes.device, gen_seed)
            if state.numel() < L.GROW_STATE_WORDS + 3 * B:
                raise ValueError("state must hold gi_grow_seeded_state_words(B) = GI_GROW_STATE_WORDS + 3 B words "
                                 "(generator.new_state(..., seeded=True))")
        elif gen_seed is not None:
            raise ValueError("generated_seed is only written with seeds")
        self.t, self.state, self.B, self.device = t, state, B, nodes.device
        self.A = 1
        for x in sub:
            self.A *= x
        d = L.GrowDesc()
        for name, _ in _STATE_TENSORS:
            field = name.replace("generated_", "gen_")
            setattr(d, field, t[name].data_ptr())
        d.state, d.host_state = state.data_ptr(), host_state
        d.B, d.N, d.Fn, d.Fe, d.L, d.C = B, N, Fn, Fe, Lc, Cg
        d.n_groups = len(groups)
        for j, g in enumerate(groups):
            d.group[j] = g
        self.desc = d

    def step(self, action: torch.Tensor, likelihood: torch.Tensor, flags: torch.Tensor) -> None:
        B = self.B
        for name, x, shape, dtype in (("action", action, (B, 4), torch.int32),
                                      ("likelihood", likelihood, (B,), torch.float32),
                                      ("flags", flags, (B,), torch.int32)):
            if not x.is_cuda or x.device != self.device:
                raise RuntimeError(f"grow_step: {name} must be a CUDA tensor on {self.device}")
            if x.dtype != dtype or tuple(x.shape) != shape or not x.is_contiguous():
                raise ValueError(f"grow_step: {name} must be contiguous {dtype} {shape} (gi_sample_actions' output)")
        d = self.desc
        d.action, d.likelihood, d.flags = action.data_ptr(), likelihood.data_ptr(), flags.data_ptr()
        st = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            if self.seed_desc is not None:
                L.check(L.load().gi_grow_graphs_seeded(C.byref(d), C.byref(self.seed_desc), st),
                        "gi_grow_graphs_seeded")
            else:
                L.check(L.load().gi_grow_graphs(C.byref(d), st), "gi_grow_graphs")

    def seed_init(self, prior_likelihoods: Optional[torch.Tensor] = None) -> None:
        """gi_grow_seed_init on the current stream: every slot but 0 starts from its seed."""
        with torch.cuda.device(self.device):
            L.check(L.load().gi_grow_seed_init(C.byref(self.desc), C.byref(self.seed_desc),
                                               None if prior_likelihoods is None else prior_likelihoods.data_ptr(),
                                               torch.cuda.current_stream(self.device).cuda_stream),
                    "gi_grow_seed_init")


def _tensors(gen) -> dict:
    return {name: getattr(gen, name) for name, _ in _STATE_TENSORS}


def grow_step(nodes, edges, n_nodes, likelihoods, generated_nodes, generated_edges, generated_n_nodes,
              generated_likelihoods, properly_terminated, action, likelihood, flags,
              dim_f_add: Sequence[int], dim_f_conn: Sequence[int], state: torch.Tensor, *,
              seeds: Optional[SeedBank] = None, generated_seed: Optional[torch.Tensor] = None) -> None:
    """One growth step (gi_grow_graphs) on the given generator tensors, in place, from ``sample_actions_raw``'s
    ``(action, likelihood, flags)``.  ``state`` (``new_state``) carries the counters from round to round: ``state[0]``
    graphs generated, ``[1]`` round, ``[2]`` target, ``[3]`` error bits (``lib.GROW_ERR_*``).

    ``seeds`` (a SeedBank): the seeded step (gi_grow_graphs_seeded) — a graph written out restarts from a seed, and
    ``generated_seed`` (int32 [C], optional) receives the seed of every generated row.  ``state`` is then
    ``new_state(..., seeded=True)`` and the tensors were filled by ``seed_init`` before the first round."""
    L.load()
    t = dict(zip((n for n, _ in _STATE_TENSORS),
                 (nodes, edges, n_nodes, likelihoods, generated_nodes, generated_edges, generated_n_nodes,
                  generated_likelihoods, properly_terminated)))
    _Grower(t, dim_f_add, dim_f_conn, state, seeds=seeds, gen_seed=generated_seed).step(action, likelihood, flags)


def seed_init(nodes, edges, n_nodes, likelihoods, state: torch.Tensor, seeds: SeedBank, *,
              prior_likelihoods: Optional[torch.Tensor] = None) -> None:
    """The first fill of seeded generation (gi_grow_seed_init), in place: slot 0 stays the dummy graph, slot
    ``g >= 1`` takes seed ``(g - 1) mod S`` (nodes, edges, n_nodes; its likelihood row — and the row of
    ``prior_likelihoods`` — zeroed), and ``state`` (``new_state(..., seeded=True)``, before the first round) records
    every slot's seed.  ``build_graphs`` / ``build_graphs_rl`` do this themselves."""
    L.load()
    if not isinstance(seeds, SeedBank):
        raise TypeError("seeds must be a generator.SeedBank")
    rows = [("nodes", nodes, torch.float32), ("edges", edges, torch.float32), ("n_nodes", n_nodes, torch.int8),
            ("likelihoods", likelihoods, torch.float32)]
    if prior_likelihoods is not None:
        rows.append(("prior_likelihoods", prior_likelihoods, torch.float32))
    for name, x, dtype in rows:
        if not x.is_cuda:
            raise RuntimeError(f"seed_init needs CUDA (ROCm) tensors ({name} is on {x.device}): the MI355X HIP path "
                               "has no CPU fallback")
        if x.dtype != dtype or not x.is_contiguous() or x.device != nodes.device:
            raise ValueError(f"{name} must be a contiguous {dtype} tensor on {nodes.device}")
    if nodes.dim() != 3 or edges.dim() != 4:
        raise ValueError("nodes must be [B, N, Fn] and edges [B, N, N, Fe]")
    B, N, Fn = nodes.shape
    Fe = edges.shape[3]
    if tuple(edges.shape) != (B, N, N, Fe) or tuple(n_nodes.shape) != (B,) or likelihoods.dim() != 2 or \
            likelihoods.shape[0] != B or likelihoods.shape[1] < 1 or \
            (prior_likelihoods is not None and prior_likelihoods.shape != likelihoods.shape):
        raise ValueError("edges / n_nodes / likelihoods do not match nodes' [B, N, Fn]")
    if state.dtype != torch.int32 or state.device != nodes.device or not state.is_contiguous() or \
            state.numel() < L.GROW_STATE_WORDS + 3 * B:
        raise ValueError("state must hold gi_grow_seeded_state_words(B) = GI_GROW_STATE_WORDS + 3 B int32 words "
                         "(generator.new_state(..., seeded=True))")
    d = L.GrowDesc()
    d.nodes, d.edges, d.n_nodes, d.likelihoods = (x.data_ptr() for x in (nodes, edges, n_nodes, likelihoods))
    d.state = state.data_ptr()
    d.B, d.N, d.Fn, d.Fe, d.L = B, N, Fn, Fe, likelihoods.shape[1]
    sd = seeds.desc(N, Fn, Fe, nodes.device, None)
    with torch.cuda.device(nodes.device):
        L.check(L.load().gi_grow_seed_init(C.byref(d), C.byref(sd),
                                           None if prior_likelihoods is None else prior_likelihoods.data_ptr(),
                                           torch.cuda.current_stream(nodes.device).cuda_stream), "gi_grow_seed_init")


class _HostMirror:
    """Four ints of mapped host memory that the step's last launch fills with state[0..3] (gi_host_flag_create)."""

    def __init__(self, target: int):
        lib = L.load()
        self.host, self.dev = C.c_void_p(), C.c_void_p()
        L.check(lib.gi_host_flag_create(C.byref(self.host), C.byref(self.dev)), "gi_host_flag_create")
        self.view = C.cast(self.host, C.POINTER(C.c_int))
        self.view[2] = int(target)

    def read(self):
        return tuple(self.view[i] for i in range(4))

    def close(self) -> None:
        if self.host:
            L.load().gi_host_flag_destroy(self.host)
            self.host = C.c_void_p()


@contextlib.contextmanager
def _host_sync_allowed():
    """The loop's own polls and its final synchronisation, under a caller's ``torch.cuda.set_sync_debug_mode``."""
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode(0)
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(prev)


def build_graphs(gen, dim_f_add: Sequence[int], dim_f_conn: Sequence[int], *, uniforms: Optional[torch.Tensor] = None,
                 generator: Optional[torch.Generator] = None, poll_every: int = 8, capture: bool = False,
                 seeds: Optional[SeedBank] = None, constraint: Optional[ActionConstraint] = None) -> int:
    """Drop-in for ``GraphGenerator.build_graphs`` (GraphGenerator.py:99-161): ``gen`` is the reference's generator
    (duck-typed: ``model``, ``batch_size`` and the tensors its ``__init__`` allocates), mutated in place; returns
    ``n_generated_so_far`` and sets ``gen.generation_rounds`` (rounds applied).

    ``uniforms`` [R, B] pins round r's draw to row r (default: ``torch.rand`` on the device from ``generator``).
    The host reads the mapped counters every ``poll_every`` rounds after waiting for the round ``poll_every``
    rounds back, never for the whole device; the result does not depend on it.  ``capture=True`` records one round
    (sync-free forward, draw, growth) into a hipGraph and replays it.  No progress bar; no autograd (the rounds run
    under ``torch.no_grad``).  Raises ``IndexError`` where the reference does (more rounds than likelihood columns),
    ``RuntimeError`` for other states it would reject.

    ``seeds`` (a SeedBank): seeded generation, in every mode.  ``gen``'s tensors are as the reference's ``__init__``
    leaves them; one launch fills slot ``g >= 1`` with seed ``(g - 1) mod S``, every graph written out restarts from
    seed ``(B - 1 + row) mod S`` (``row`` its index in ``generated_*``), and ``gen.generated_seed`` (int32 [C], on the
    device, -1 past the rows written) names the seed each generated row was grown from.  The generated likelihood
    rows hold the actions sampled after the (re)start only: the likelihood of the completion given the seed.

    ``constraint`` (a ``sampler.ActionConstraint``): constrained generation, in every mode and together with ``seeds``.
    One more launch per round (``gi_action_mask``, part of the captured round and of its warm-up) sets every
    inadmissible action to -inf in a copy of the logits, and the draw is taken from the renormalised distribution: no
    attach to an empty slot, no second bond on a pair, no add to a full graph, no atom over the largest valence of
    the rules' table (the library's own, not RDKit's).  With valid seeds every generated row is then valid under
    ``analyze.validity`` and properly terminated.  **The likelihoods written are those of the constrained policy**, not
    the unconstrained model's (``likelihood.molecule_log_likelihood`` still scores the latter).  A molecule can take
    more actions than ``2 N``: size the likelihood columns for it, or the documented ``IndexError`` is raised.
    ``gen.constraint_stats`` (device tensors, nothing read back in the loop): ``rounds`` applied,
    ``graph_rounds_masked`` (graph-rounds in which probability mass was removed) and ``mass_removed`` (its sum),
    graph 0 left out.  ``None`` (the default) adds no launch."""
    if poll_every < 1:
        raise ValueError("poll_every must be >= 1")
    model, B = gen.model, int(gen.batch_size)
    t = _tensors(gen)
    dev = t["nodes"].device
    if not t["nodes"].is_cuda:
        raise RuntimeError("build_graphs needs the generator's tensors on a CUDA (ROCm) device: the MI355X HIP path "
                           "has no CPU fallback")
    if uniforms is not None:
        if uniforms.dim() != 2 or uniforms.shape[1] != B:
            raise ValueError(f"uniforms must be [R, {B}], got {tuple(uniforms.shape)}")
        with _host_sync_allowed():                       # (set-up: a host tensor's upload may synchronise)
            uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
    state = new_state(B, B, dev, seeded=seeds is not None)
    gen_seed = None
    if seeds is not None:
        gen_seed = torch.full((t["generated_nodes"].shape[0],), -1, dtype=torch.int32, device=dev)
    mirror = _HostMirror(B)
    try:
        grower = _Grower(t, dim_f_add, dim_f_conn, state, mirror.dev.value, seeds, gen_seed)
        masker = _Masker(constraint, t, state) if constraint is not None else None
    except Exception:
        mirror.close()
        raise
    nodes, edges, n_nodes, A = t["nodes"], t["edges"], t["n_nodes"], grower.A
    if masker is None:
        logits_of = lambda warm=False: model(nodes, edges)                              # noqa: E731
    else:
        logits_of = lambda warm=False: masker.raw(model(nodes, edges), not warm)        # noqa: E731
    stream = torch.cuda.current_stream(dev)
    sync_free = capture or bool(getattr(model, "sync_free", False))
    prev_sync_free = getattr(model, "sync_free", None)
    graph = None
    try:
        with torch.no_grad(), torch.cuda.device(dev):
            if seeds is not None:
                grower.seed_init()
            if capture:
                model.sync_free = True
                u_buf = torch.zeros(B, dtype=torch.float32, device=dev)
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(stream)
                with torch.cuda.stream(side):            # warm-up: the model's persistent device state; no round applied
                    sample_actions_raw(logits_of(True), n_nodes, edges, A, uniform=u_buf)
                stream.wait_stream(side)
                with _host_sync_allowed():                   # (set-up: the capture synchronises on entry)
                    torch.cuda.synchronize(dev)
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        grower.step(*sample_actions_raw(logits_of(), n_nodes, edges, A, uniform=u_buf))
            pending = collections.deque()
            r = 0
            while uniforms is None or r < uniforms.shape[0]:
                if capture:
                    if uniforms is not None:
                        u_buf.copy_(uniforms[r])
                    else:
                        u_buf.uniform_(generator=generator)
                    graph.replay()
                else:
                    u = uniforms[r] if uniforms is not None else torch.rand(B, device=dev, generator=generator)
                    grower.step(*sample_actions_raw(logits_of(), n_nodes, edges, A, uniform=u))
                r += 1
                ev = torch.cuda.Event()
                ev.record(stream)
                pending.append(ev)
                if r % poll_every == 0:
                    with _host_sync_allowed():
                        last = None
                        while len(pending) > poll_every:
                            last = pending.popleft()
                        if last is not None:
                            last.synchronize()       # at most poll_every rounds in flight
                    n, _, target, err = mirror.read()
                    if n >= target or err:
                        break
            with _host_sync_allowed():
                stream.synchronize()
                n, rounds, target, err = (int(x) for x in state[:4].cpu())
                if sync_free and hasattr(model, "last_bounded_error"):
                    model.last_bounded_error()
    finally:
        if prev_sync_free is not None:
            model.sync_free = prev_sync_free
        with _host_sync_allowed():
            del graph
            mirror.close()
    gen.generation_rounds = rounds
    if seeds is not None:
        gen.generated_seed = gen_seed
    if masker is not None:
        gen.constraint_stats = masker.stats
    _raise_for_outcome("build_graphs", n, rounds, target, err, t["likelihoods"], uniforms)
    return n


def _raise_for_outcome(what: str, n: int, rounds: int, target: int, err: int, likelihoods: torch.Tensor,
                       uniforms: Optional[torch.Tensor]) -> None:
    """The reference's exceptions for a loop's final counters: IndexError past the last likelihood column,
    RuntimeError for the other rejected states and for pinned uniforms that ran out."""
    if err & L.GROW_ERR_ROUND:
        raise IndexError(f"{what}: generation round {rounds} has no likelihood column "
                         f"(likelihoods has {likelihoods.shape[1]})")
    if err:
        raise RuntimeError("%s: the growth step rejected round %d: %s" % (what, rounds, ", ".join(
            m for bit, m in ((L.GROW_ERR_CAPACITY, "more finished graphs than generated_* rows"),
                             (L.GROW_ERR_ACTION, "an action index out of range"),
                             (L.GROW_ERR_NNODES, "n_nodes overflows int8")) if err & bit)))
    if n < target:
        raise RuntimeError(f"{what}: the {uniforms.shape[0]} rows of uniforms ran out after {rounds} rounds "
                           f"with {n} of {target} graphs generated")


# ---- RL fine-tuning (GraphGeneratorRL.build_graphs) ----------------------------------------------------------------

def _tensors_rl(gen) -> dict:
    """GraphGeneratorRL's tensors under gi_grow_desc's names (the agent's likelihood stream as the base one)."""
    t = {name: getattr(gen, name) for name, _ in _STATE_TENSORS
         if name not in ("likelihoods", "generated_likelihoods")}
    t["likelihoods"], t["generated_likelihoods"] = gen.agent_likelihoods, gen.generated_agent_likelihoods
    return t


def _validate_rl(t: dict, prior: Sequence[torch.Tensor], dim_f_add: Sequence[int], dim_f_conn: Sequence[int]):
    """_validate with the prior's (likelihoods, generated_likelihoods) checked like the agent's, in the same order
    (dtypes and layout, shapes, then the device)."""
    pairs = (("prior_likelihoods", prior[0], t["likelihoods"]),
             ("generated_prior_likelihoods", prior[1], t["generated_likelihoods"]))
    for name, x, _ in pairs:
        if x.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32 (the reference's dtype), got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous: the step writes it in place")
    for name, x, like in pairs:
        if x.shape != like.shape:
            raise ValueError(f"{name} has shape {tuple(x.shape)}, expected {tuple(like.shape)}")
    dims, sub, groups = _validate(t, dim_f_add, dim_f_conn)
    for name, x, like in pairs:
        if x.device != like.device:
            raise ValueError(f"{name} is on {x.device}, the agent's on {like.device}")
    return dims, sub, groups


class _GrowerRL(_Grower):
    """Validated gi_grow_rl_desc: the agent's stream in ``t``, the prior's in ``prior`` (likelihoods, generated
    likelihoods), the trajectory record in ``traj`` (int32 [3, C] or None)."""

    def __init__(self, t: dict, prior: Sequence[torch.Tensor], traj: Optional[torch.Tensor],
                 dim_f_add: Sequence[int], dim_f_conn: Sequence[int], state: torch.Tensor,
                 host_state: Optional[int] = None, seeds: Optional[SeedBank] = None,
                 gen_seed: Optional[torch.Tensor] = None):
        (B, _, _, _, _, Cg), _, _ = _validate_rl(t, prior, dim_f_add, dim_f_conn)
        super().__init__(t, dim_f_add, dim_f_conn, state, host_state, seeds, gen_seed)
        if state.numel() < L.GROW_STATE_WORDS + 2 * B:
            raise ValueError("state must hold gi_grow_rl_state_words(B) = GI_GROW_STATE_WORDS + 2 B words "
                             "(generator.new_state(..., rl=True))")
        if traj is not None and (traj.dtype != torch.int32 or tuple(traj.shape) != (3, Cg) or
                                 not traj.is_contiguous() or traj.device != self.device):
            raise ValueError(f"traj must be a contiguous int32 [3, {Cg}] tensor on {self.device}")
        self.prior, self.traj = prior, traj
        d = L.GrowRlDesc()
        d.base = self.desc
        d.prior_likelihoods, d.gen_prior_likelihoods = prior[0].data_ptr(), prior[1].data_ptr()
        d.traj = traj.data_ptr() if traj is not None else None
        self.desc_rl = d

    def step(self, action: torch.Tensor, like_agent: torch.Tensor, like_prior: torch.Tensor,
             flags: torch.Tensor) -> None:
        B = self.B
        for name, x, shape, dtype in (("action", action, (B, 4), torch.int32),
                                      ("like_agent", like_agent, (B,), torch.float32),
                                      ("like_prior", like_prior, (B,), torch.float32),
                                      ("flags", flags, (B,), torch.int32)):
            if not x.is_cuda or x.device != self.device:
                raise RuntimeError(f"grow_step_rl: {name} must be a CUDA tensor on {self.device}")
            if x.dtype != dtype or tuple(x.shape) != shape or not x.is_contiguous():
                raise ValueError(f"grow_step_rl: {name} must be contiguous {dtype} {shape} "
                                 "(gi_sample_actions_rl's output)")
        d = self.desc_rl
        d.base.action, d.base.likelihood, d.base.flags = action.data_ptr(), like_agent.data_ptr(), flags.data_ptr()
        d.prior_likelihood = like_prior.data_ptr()
        st = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            if self.seed_desc is not None:
                L.check(L.load().gi_grow_graphs_rl_seeded(C.byref(d), C.byref(self.seed_desc), st),
                        "gi_grow_graphs_rl_seeded")
            else:
                L.check(L.load().gi_grow_graphs_rl(C.byref(d), st), "gi_grow_graphs_rl")


def grow_step_rl(nodes, edges, n_nodes, agent_likelihoods, prior_likelihoods, generated_nodes, generated_edges,
                 generated_n_nodes, generated_agent_likelihoods, generated_prior_likelihoods, properly_terminated,
                 action, like_agent, like_prior, flags, dim_f_add: Sequence[int], dim_f_conn: Sequence[int],
                 state: torch.Tensor, traj: Optional[torch.Tensor] = None, *, seeds: Optional[SeedBank] = None,
                 generated_seed: Optional[torch.Tensor] = None) -> None:
    """One RL growth step (gi_grow_graphs_rl) on GraphGeneratorRL's tensors, in place, from
    ``sample_actions_rl_raw``'s ``(action, like_agent, like_prior, flags)``.  ``state`` = ``new_state(..., rl=True)``;
    ``traj`` (int32 [3, C], optional) receives each generated row's source graph, first and last round.
    ``seeds`` / ``generated_seed``: the seeded step (gi_grow_graphs_rl_seeded), as in ``grow_step``."""
    L.load()
    t = dict(nodes=nodes, edges=edges, n_nodes=n_nodes, likelihoods=agent_likelihoods,
             generated_nodes=generated_nodes, generated_edges=generated_edges, generated_n_nodes=generated_n_nodes,
             generated_likelihoods=generated_agent_likelihoods, properly_terminated=properly_terminated)
    _GrowerRL(t, (prior_likelihoods, generated_prior_likelihoods), traj, dim_f_add, dim_f_conn,
              state, seeds=seeds, gen_seed=generated_seed).step(action, like_agent, like_prior, flags)


def traj_gather(like_agent: Optional[torch.Tensor], like_prior: Optional[torch.Tensor], traj: torch.Tensor, n: int,
                L_cols: int):
    """gi_grow_traj_gather: the generated likelihood rows [C, L_cols] of both sides from the per-round likelihoods
    [R, B] (a side given as None is skipped and returned as None)."""
    lib = L.load()
    ref = like_agent if like_agent is not None else like_prior
    R, B = ref.shape
    Cg = traj.shape[1]
    ins = [x.detach().float().contiguous() if x is not None else None for x in (like_agent, like_prior)]
    outs = [torch.empty((Cg, L_cols), dtype=torch.float32, device=ref.device) if x is not None else None
            for x in ins]
    ptr = lambda x: x.data_ptr() if x is not None else None
    with torch.cuda.device(ref.device):
        L.check(lib.gi_grow_traj_gather(n, R, B, Cg, L_cols, traj.data_ptr(), ptr(ins[0]), ptr(ins[1]),
                                        ptr(outs[0]), ptr(outs[1]), torch.cuda.current_stream(ref.device).cuda_stream),
                "gi_grow_traj_gather")
    return outs[0], outs[1]


def traj_scatter(g_agent: Optional[torch.Tensor], g_prior: Optional[torch.Tensor], traj: torch.Tensor, n: int,
                 R: int, B: int):
    """gi_grow_traj_scatter: the gradients [R, B] of the per-round likelihoods from those of the generated rows
    [C, L] (a side given as None is skipped and returned as None)."""
    lib = L.load()
    ref = g_agent if g_agent is not None else g_prior
    Cg, L_cols = ref.shape
    gs = [x.float().contiguous() if x is not None else None for x in (g_agent, g_prior)]
    outs = [torch.empty((R, B), dtype=torch.float32, device=ref.device) if x is not None else None for x in gs]
    ptr = lambda x: x.data_ptr() if x is not None else None
    with torch.cuda.device(ref.device):
        L.check(lib.gi_grow_traj_scatter(n, R, B, Cg, L_cols, traj.data_ptr(), ptr(gs[0]), L_cols, ptr(gs[1]),
                                         L_cols, ptr(outs[0]), ptr(outs[1]),
                                         torch.cuda.current_stream(ref.device).cuda_stream),
                "gi_grow_traj_scatter")
    return outs[0], outs[1]


class _TrajGather(torch.autograd.Function):
    """The generated likelihood rows of both sides as a differentiable function of the per-round likelihoods."""

    @staticmethod
    def forward(ctx, like_agent, like_prior, traj, n, L_cols):
        ctx.set_materialize_grads(False)
        gen_a, gen_p = traj_gather(like_agent, like_prior, traj, n, L_cols)
        ctx.save_for_backward(traj)
        ctx.n, ctx.RB = n, tuple(like_agent.shape)
        for needs, out in zip(ctx.needs_input_grad[:2], (gen_a, gen_p)):
            if not needs:
                ctx.mark_non_differentiable(out)
        return gen_a, gen_p

    @staticmethod
    def backward(ctx, g_agent, g_prior):
        (traj,) = ctx.saved_tensors
        g_a = g_agent if ctx.needs_input_grad[0] else None
        g_p = g_prior if ctx.needs_input_grad[1] else None
        if g_a is None and g_p is None:
            return (None,) * 5
        d_a, d_p = traj_scatter(g_a, g_p, traj, ctx.n, *ctx.RB)
        return d_a, d_p, None, None, None


def build_graphs_rl(gen, dim_f_add: Sequence[int], dim_f_conn: Sequence[int], *,
                    uniforms: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                    poll_every: int = 1, seeds: Optional[SeedBank] = None,
                    constraint: Optional[ActionConstraint] = None) -> int:
    """Drop-in for ``GraphGeneratorRL.build_graphs`` (GraphGeneratorRL.py:109-172): ``gen`` is the reference's RL
    generator (duck-typed: ``agent_model``, ``prior_model``, ``batch_size`` and the tensors of its
    ``allocate_graph_tensors`` / ``initialize_graph_batch``), mutated in place; returns ``n_generated_so_far`` and
    sets ``gen.generation_rounds`` (rounds applied).

    Every round runs both forwards with grad, ``sample_actions_rl``'s draw (no index tuples) and
    ``gi_grow_graphs_rl``; nothing is read back inside a round but the forwards' own counts.
    ``gen.generated_agent_likelihoods`` / ``gen.generated_prior_likelihoods`` are then REPLACED by the outputs of an
    autograd Function over the stacked likelihoods of the applied rounds (rounds enqueued past the target are not in
    the graph), with the values the step wrote in place; ``agent_likelihoods`` / ``prior_likelihoods`` hold their
    values without an autograd graph.  ``uniforms``, ``generator`` and the exceptions are ``build_graphs``'.  The host
    reads the mapped counters every ``poll_every`` rounds after waiting for the round ``poll_every - 1`` rounds back:
    every round already waits for its forwards' counts, so the default 1 costs a short wait per round and enqueues
    no round past the target (each would cost two forwards with grad); the result does not depend on it.

    ``seeds`` (a SeedBank): seeded generation as in ``build_graphs`` — the first fill, restarts from seed
    ``(B - 1 + row) mod S``, ``gen.generated_seed``; both likelihood streams and their gradients are those of the
    completions given the seeds.

    ``constraint`` (a ``sampler.ActionConstraint``): constrained generation as in ``build_graphs`` — ONE mask launch per
    round writes the masked copies of the agent's and the prior's logits, the draw is taken from the agent's
    renormalised distribution, and BOTH likelihood streams are those of the constrained policies.  The gradients reach
    the models through the mask: the sampler's backward already writes exact zeros at masked columns, so the mask
    hands its upstream gradient through.  ``gen.constraint_stats`` as in ``build_graphs`` (of the agent's logits)."""
    if poll_every < 1:
        raise ValueError("poll_every must be >= 1")
    agent, prior, B = gen.agent_model, gen.prior_model, int(gen.batch_size)
    t = _tensors_rl(gen)
    prior_t = (gen.prior_likelihoods, gen.generated_prior_likelihoods)
    _validate_rl(t, prior_t, dim_f_add, dim_f_conn)          # TypeError / ValueError / RuntimeError before any launch
    dev = t["nodes"].device
    if uniforms is not None:
        if uniforms.dim() != 2 or uniforms.shape[1] != B:
            raise ValueError(f"uniforms must be [R, {B}], got {tuple(uniforms.shape)}")
        with _host_sync_allowed():
            uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
    Cg, L_cols = t["generated_likelihoods"].shape
    state = new_state(B, B, dev, rl=True, seeded=seeds is not None)
    traj = torch.zeros((3, Cg), dtype=torch.int32, device=dev)
    gen_seed = torch.full((Cg,), -1, dtype=torch.int32, device=dev) if seeds is not None else None
    mirror = _HostMirror(B)
    try:
        grower = _GrowerRL(t, prior_t, traj, dim_f_add, dim_f_conn, state, mirror.dev.value, seeds, gen_seed)
        masker = _Masker(constraint, t, state) if constraint is not None else None
        nodes, edges, n_nodes, A = t["nodes"], t["edges"], t["n_nodes"], grower.A
        stream = torch.cuda.current_stream(dev)
        likes_a, likes_p = [], []
        with torch.cuda.device(dev):
            if seeds is not None:
                with torch.no_grad():
                    grower.seed_init(prior_t[0])
            pending = collections.deque()
            r = 0
            while uniforms is None or r < uniforms.shape[0]:
                u = uniforms[r] if uniforms is not None else torch.rand(B, device=dev, generator=generator)
                out_a, out_p = agent(nodes, edges), prior(nodes, edges)
                if masker is not None:
                    out_a, out_p = masker.rl(out_a, out_p)
                action, like_a, like_p, flags = _SampleRL.apply(out_a, out_p, n_nodes, edges, A, u, None)
                grower.step(action, like_a, like_p, flags)
                likes_a.append(like_a)
                likes_p.append(like_p)
                r += 1
                ev = torch.cuda.Event()
                ev.record(stream)
                pending.append(ev)
                if r % poll_every == 0:
                    with _host_sync_allowed():
                        last = None
                        while len(pending) > poll_every - 1:
                            last = pending.popleft()
                        if last is not None:
                            last.synchronize()
                    n, _, target, err = mirror.read()
                    if n >= target or err:
                        break
            with _host_sync_allowed():
                stream.synchronize()
                n, rounds, target, err = (int(x) for x in state[:4].cpu())
    finally:
        with _host_sync_allowed():
            mirror.close()
    gen.generation_rounds = rounds
    if seeds is not None:
        gen.generated_seed = gen_seed
    if masker is not None:
        gen.constraint_stats = masker.stats
    _raise_for_outcome("build_graphs_rl", n, rounds, target, err, t["likelihoods"], uniforms)
    del likes_a[rounds:], likes_p[rounds:]               # frozen rounds leave the autograd graph with these
    gen_a, gen_p = _TrajGather.apply(torch.stack(likes_a), torch.stack(likes_p), traj, n, L_cols)
    gen.generated_agent_likelihoods, gen.generated_prior_likelihoods = gen_a, gen_p
    return n
