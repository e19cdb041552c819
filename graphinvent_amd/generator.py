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
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
from typing import Optional, Sequence

import torch

from . import lib as L
from .sampler import _add_dims, sample_actions_raw

#: the generator tensors the step reads and writes, in gi_grow_desc's order, with their dtypes
_STATE_TENSORS = (("nodes", torch.float32), ("edges", torch.float32), ("n_nodes", torch.int8),
                  ("likelihoods", torch.float32), ("generated_nodes", torch.float32),
                  ("generated_edges", torch.float32), ("generated_n_nodes", torch.int8),
                  ("generated_likelihoods", torch.float32), ("properly_terminated", torch.int8))


def new_state(batch_size: int, target: int, device) -> torch.Tensor:
    """The step's device state: int32 [GI_GROW_STATE_WORDS + B], zero with ``state[2] = target``."""
    state = torch.zeros(L.GROW_STATE_WORDS + batch_size, dtype=torch.int32, device=device)
    state.narrow(0, 2, 1).fill_(int(target))          # a fill launch: no host -> device copy
    return state


class _Grower:
    """Validated gi_grow_desc of one set of generator tensors; ``step`` enqueues one round."""

    def __init__(self, t: dict, dim_f_add: Sequence[int], dim_f_conn: Sequence[int], state: torch.Tensor,
                 host_state: Optional[int] = None):
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
        if state.dtype != torch.int32 or state.device != nodes.device or not state.is_contiguous() or \
                state.numel() < L.GROW_STATE_WORDS + B:
            raise ValueError("state must be a contiguous int32 tensor of GI_GROW_STATE_WORDS + B words on the "
                             "tensors' device (generator.new_state)")
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
        with torch.cuda.device(self.device):
            L.check(L.load().gi_grow_graphs(C.byref(d), torch.cuda.current_stream(self.device).cuda_stream),
                    "gi_grow_graphs")


def _tensors(gen) -> dict:
    return {name: getattr(gen, name) for name, _ in _STATE_TENSORS}


def grow_step(nodes, edges, n_nodes, likelihoods, generated_nodes, generated_edges, generated_n_nodes,
              generated_likelihoods, properly_terminated, action, likelihood, flags,
              dim_f_add: Sequence[int], dim_f_conn: Sequence[int], state: torch.Tensor) -> None:
    """One growth step (gi_grow_graphs) on the given generator tensors, in place, from ``sample_actions_raw``'s
    ``(action, likelihood, flags)``.  ``state`` (``new_state``) carries the counters from round to round: ``state[0]``
    graphs generated, ``[1]`` round, ``[2]`` target, ``[3]`` error bits (``lib.GROW_ERR_*``)."""
    L.load()
    t = dict(zip((n for n, _ in _STATE_TENSORS),
                 (nodes, edges, n_nodes, likelihoods, generated_nodes, generated_edges, generated_n_nodes,
                  generated_likelihoods, properly_terminated)))
    _Grower(t, dim_f_add, dim_f_conn, state).step(action, likelihood, flags)


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
                 generator: Optional[torch.Generator] = None, poll_every: int = 8, capture: bool = False) -> int:
    """Drop-in for ``GraphGenerator.build_graphs`` (GraphGenerator.py:99-161): ``gen`` is the reference's generator
    (duck-typed: ``model``, ``batch_size`` and the tensors its ``__init__`` allocates), mutated in place; returns
    ``n_generated_so_far`` and sets ``gen.generation_rounds`` (rounds applied).

    ``uniforms`` [R, B] pins round r's draw to row r (default: ``torch.rand`` on the device from ``generator``).
    The host reads the mapped counters every ``poll_every`` rounds after waiting for the round ``poll_every``
    rounds back, never for the whole device; the result does not depend on it.  ``capture=True`` records one round
    (sync-free forward, draw, growth) into a hipGraph and replays it.  No progress bar; no autograd (the rounds run
    under ``torch.no_grad``).  Raises ``IndexError`` where the reference does (more rounds than likelihood columns),
    ``RuntimeError`` for other states it would reject."""
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
    state = new_state(B, B, dev)
    mirror = _HostMirror(B)
    grower = _Grower(t, dim_f_add, dim_f_conn, state, mirror.dev.value)
    nodes, edges, n_nodes, A = t["nodes"], t["edges"], t["n_nodes"], grower.A
    stream = torch.cuda.current_stream(dev)
    sync_free = capture or bool(getattr(model, "sync_free", False))
    prev_sync_free = getattr(model, "sync_free", None)
    graph = None
    try:
        with torch.no_grad(), torch.cuda.device(dev):
            if capture:
                model.sync_free = True
                u_buf = torch.zeros(B, dtype=torch.float32, device=dev)
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(stream)
                with torch.cuda.stream(side):            # warm-up: the model's persistent device state; no round applied
                    sample_actions_raw(model(nodes, edges), n_nodes, edges, A, uniform=u_buf)
                stream.wait_stream(side)
                with _host_sync_allowed():                   # (set-up: the capture synchronises on entry)
                    torch.cuda.synchronize(dev)
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        grower.step(*sample_actions_raw(model(nodes, edges), n_nodes, edges, A, uniform=u_buf))
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
                    grower.step(*sample_actions_raw(model(nodes, edges), n_nodes, edges, A, uniform=u))
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
    if err & L.GROW_ERR_ROUND:
        raise IndexError(f"build_graphs: generation round {rounds} has no likelihood column "
                         f"(likelihoods has {t['likelihoods'].shape[1]})")
    if err:
        raise RuntimeError("build_graphs: the growth step rejected round %d: %s" % (rounds, ", ".join(
            m for bit, m in ((L.GROW_ERR_CAPACITY, "more finished graphs than generated_* rows"),
                             (L.GROW_ERR_ACTION, "an action index out of range"),
                             (L.GROW_ERR_NNODES, "n_nodes overflows int8")) if err & bit)))
    if n < target:
        raise RuntimeError(f"build_graphs: the {uniforms.shape[0]} rows of uniforms ran out after {rounds} rounds "
                           f"with {n} of {target} graphs generated")
    return n
