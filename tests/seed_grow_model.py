"""Test infrastructure: a numpy model of SEEDED generation (gi_grow_seed_init, gi_grow_graphs_seeded;
include/graphinvent_amd.h) on top of tests/grow_oracle.py, which it imports and does not change.

A seeded round is ``grow_oracle.grow_round`` followed by the refill: the graph written to generated row ``row``
restarts from seed ``(B - 1 + row) mod S`` of the bank instead of from zeros, and ``gen_seed[row]`` receives the seed
the slot was grown from.  The first fill gives slot ``g >= 1`` seed ``(g - 1) mod S``; slot 0 stays the dummy graph
(seed -1).  A bank is a dict of int8 arrays ``nodes [S, N, Fn]``, ``edges [S, N, N, Fe]``, ``n_nodes [S]``."""
import numpy as np
import torch

from oracle import callers_oracle as CO
from oracle import sampler_oracle as SO
from tests import grow_oracle as GO


def empty_bank(N, Fn, Fe, S=1):
    return dict(nodes=np.zeros((S, N, Fn), np.int8), edges=np.zeros((S, N, N, Fe), np.int8),
                n_nodes=np.zeros(S, np.int8))


def chain_seed(N, groups, Fe, n, rng):
    """A valid seed of ``n`` atoms (0 <= n <= N): random atom features, node i > 0 bonded to a random earlier node,
    plus, where there is room, one ring-closing bond."""
    Fn = sum(groups)
    nodes, edges = np.zeros((N, Fn), np.int8), np.zeros((N, N, Fe), np.int8)
    offs = np.concatenate([[0], np.cumsum(groups)[:-1]])
    for i in range(n):
        for off, size in zip(offs, groups):
            nodes[i, off + rng.integers(size)] = 1
        if i:
            j, b = rng.integers(i), rng.integers(Fe)
            edges[i, j, b] = edges[j, i, b] = 1
    if n >= 3:
        free = [(i, j) for i in range(n) for j in range(i) if not edges[i, j].any()]
        if free:
            i, j = free[rng.integers(len(free))]
            b = rng.integers(Fe)
            edges[i, j, b] = edges[j, i, b] = 1
    return nodes, edges


def mixed_bank(N, groups, Fe, S, seed=0):
    """S seeds: the empty seed, a one-atom seed, a full seed (n_nodes = N) and sizes in between, cycled (S = 1: one
    seed of two atoms)."""
    rng = np.random.default_rng([seed, N, S])
    sizes = [2] if S == 1 else [0, 1, N] + [2 + k % max(N - 2, 1) for k in range(N)]
    mols = [chain_seed(N, groups, Fe, min(sizes[s % len(sizes)], N), rng) for s in range(S)]
    nodes, edges = np.stack([m[0] for m in mols]), np.stack([m[1] for m in mols])
    return dict(nodes=nodes, edges=edges, n_nodes=nodes.any(axis=2).sum(axis=1).astype(np.int8))


def new_seeded_state(B, N, Fn, Fe, L, C, bank):
    """``grow_oracle.new_state`` after gi_grow_seed_init, with ``slot_seed [B]`` and ``gen_seed [C]`` (-1: not
    written)."""
    s = GO.new_state(B, N, Fn, Fe, L, C)
    S = len(bank["n_nodes"])
    s["slot_seed"] = np.full(B, -1, np.int32)
    s["gen_seed"] = np.full(C, -1, np.int32)
    for g in range(1, B):
        _fill(s, g, (g - 1) % S, bank)
    return s


def _fill(s, g, seed, bank):
    s["nodes"][g] = bank["nodes"][seed]
    s["edges"][g] = bank["edges"][seed]
    s["n_nodes"][g] = bank["n_nodes"][seed]
    s["likelihoods"][g] = 0
    s["slot_seed"][g] = seed


def seeded_round(s, action, like, flags, groups, Fe, bank):
    """One gi_grow_graphs_seeded round on ``s`` (mutated): grow_round, then the refill and gen_seed."""
    B = s["nodes"].shape[0]
    n0, r0 = s["n"], s["round"]
    g = np.arange(B)
    T = g[action[:, 0] == 2]
    S = np.concatenate([T[T != 0], g[((flags & 1) != 0) & (g != 0)]])        # grow_round's S, in its order
    GO.grow_round(s, action, like, flags, groups, Fe)
    if s["round"] == r0:                                                     # frozen or refused: nothing written
        return
    assert s["n"] == n0 + len(S)
    n_seeds = len(bank["n_nodes"])
    for k, slot in enumerate(S):
        row = n0 + k
        s["gen_seed"][row] = s["slot_seed"][slot]
        _fill(s, slot, (B - 1 + row) % n_seeds, bank)


def run_seeded_oracle(cfg, bank, max_rounds=4096):
    """``grow_oracle.run_oracle`` with a seed bank: (state, draws)."""
    N, groups, Fe, dim_f_add, dim_f_conn = GO.config_dims(cfg)
    B = int(cfg["B"])
    s = new_seeded_state(B, N, sum(groups), Fe, 2 * N, 2 * B, bank)
    draw = CO.InverseCdfDraws(int(cfg["draw_seed"]), B, max_rounds)
    while s["n"] < s["target"] and not s["error"]:
        apd = torch.softmax(torch.from_numpy(GO.stub_logits(cfg, s["round"])), dim=1).numpy()
        out = SO.get_actions(apd, draw(apd), s["n_nodes"].astype(np.int64), s["edges"], dim_f_add, dim_f_conn)
        action, flags = GO.actions_from_tuples(out, B, dim_f_add)
        seeded_round(s, action, out["likelihoods"].astype(np.float32), flags, groups, Fe, bank)
    return s, draw
