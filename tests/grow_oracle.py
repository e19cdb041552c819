"""Test infrastructure: a numpy restatement of one round of ``gi_grow_graphs`` (include/graphinvent_amd.h) in the
sampler's action / flags form, the stub model of tests/golden/golden_grow.npz, and a CPU driver of the whole
``GraphGenerator.build_graphs`` loop (GraphGenerator.py:99-161) on top of ``oracle/sampler_oracle.py``.

The spec, per round, with n = graphs generated and r = round at entry:
frozen when n >= target or error != 0; T = kind == 2 (graph 0 included), I = flags & 1, S = (T without 0) + (I without
0); properly_terminated[n : n + |T|] = 1; S[k] is copied to generated row n + k after likelihoods[S[k], r] is written;
every graph's action is applied; S is reset; graph 0 is restored; n += |S|, r += 1.  Indices the reference rejects
write nothing and set an error bit (the GI_GROW_ERR_* values)."""
import numpy as np
import torch

from oracle import callers_oracle as CO
from oracle import sampler_oracle as SO

ERR_ROUND, ERR_CAPACITY, ERR_ACTION, ERR_NNODES = 1, 2, 4, 8


def new_state(B, N, Fn, Fe, L, C):
    """The reference's tensors after ``GraphGenerator.__init__`` (:27-43, 163-209, 389-428), as numpy arrays."""
    s = dict(nodes=np.zeros((B, N, Fn), np.float32), edges=np.zeros((B, N, N, Fe), np.float32),
             n_nodes=np.zeros(B, np.int8), likelihoods=np.zeros((B, L), np.float32),
             generated_nodes=np.zeros((C, N, Fn), np.float32), generated_edges=np.zeros((C, N, N, Fe), np.float32),
             generated_n_nodes=np.zeros(C, np.int8), generated_likelihoods=np.zeros((C, L), np.float32),
             properly_terminated=np.zeros(C, np.int8), n=0, round=0, target=B, error=0)
    s["nodes"][0] = 1
    s["edges"][0, 0, 0, 0] = 1
    s["n_nodes"][0] = 1
    return s


def grow_round(s, action, like, flags, groups, Fe):
    """One gi_grow_graphs round on the state dict ``s`` (mutated).  action [B, 4] = (kind, node_to, rem, from)."""
    if s["n"] >= s["target"] or s["error"]:
        return
    B, N, Fn = s["nodes"].shape
    L, C = s["likelihoods"].shape[1], s["generated_nodes"].shape[0]
    n, r = s["n"], s["round"]
    kind, to, rem, frm = (action[:, k].astype(np.int64) for k in range(4))
    inv = (flags & 1) != 0
    A = int(np.prod(groups)) * Fe
    g = np.arange(B)
    bits = 0
    if np.any((kind < 0) | (kind > 2)) or np.any((kind == 2) & inv):
        bits |= ERR_ACTION
    add, conn = kind == 0, kind == 1
    if np.any(add & ((to < 0) | (to >= N) | (rem < 0) | (rem >= A) | (frm < 0) | (frm >= N))):
        bits |= ERR_ACTION
    if np.any(conn & ((to < 0) | (to >= N) | (rem < 0) | (rem >= Fe) | (frm < -1) | (frm >= N))):
        bits |= ERR_ACTION
    if np.any(add & ~inv & (g != 0) & (s["n_nodes"].astype(np.int64) >= 127)):
        bits |= ERR_NNODES
    T = g[kind == 2]
    S = np.concatenate([T[T != 0], g[inv & (g != 0)]])
    if r >= L:
        bits |= ERR_ROUND
    if n + len(S) > C:
        bits |= ERR_CAPACITY
    if bits:
        s["error"] |= bits
        return
    s["properly_terminated"][n:min(n + len(T), C)] = 1
    s["likelihoods"][S, r] = like[S]
    rows = slice(n, n + len(S))
    for src, dst in (("nodes", "generated_nodes"), ("edges", "generated_edges"), ("n_nodes", "generated_n_nodes"),
                     ("likelihoods", "generated_likelihoods")):
        s[dst][rows] = s[src][S]
    offs = np.concatenate([[0], np.cumsum(groups)[:-1]])
    for b in range(B):
        if kind[b] == 0:
            q, bt = divmod(int(rem[b]), Fe)
            sub = np.unravel_index(q, groups)
            for j in range(len(groups)):
                s["nodes"][b, frm[b], offs[j] + sub[j]] = 1
            if s["n_nodes"][b] != 0:
                s["edges"][b, to[b], frm[b], bt] = 1
                s["edges"][b, frm[b], to[b], bt] = 1
            s["n_nodes"][b] += 1
            s["likelihoods"][b, r] = like[b]
        elif kind[b] == 1:
            f = frm[b] + N if frm[b] < 0 else frm[b]
            s["edges"][b, f, to[b], rem[b]] = 1
            s["edges"][b, to[b], f, rem[b]] = 1
            s["likelihoods"][b, r] = like[b]
    for name in ("nodes", "edges", "n_nodes", "likelihoods"):
        s[name][S] = 0
    s["nodes"][0] = 1
    s["edges"][0, 0, 0, 0] = 1
    s["n_nodes"][0] = 1
    s["n"] += len(S)
    s["round"] += 1


def actions_from_tuples(out, B, dim_f_add):
    """``sampler_oracle.get_actions``' tuples -> (action [B, 4] int32, flags [B] int32), gi_sample_actions' layout."""
    action = np.zeros((B, 4), np.int32)
    flags = np.zeros(B, np.int32)
    add, conn = out["add"], out["conn"]
    action[add[0], 0] = 0
    action[add[0], 1] = add[1]
    action[add[0], 2] = np.ravel_multi_index(tuple(add[2:-1]), tuple(dim_f_add[1:]))
    action[add[0], 3] = add[-1]
    action[conn[0], 0] = 1
    action[conn[0], 1], action[conn[0], 2], action[conn[0], 3] = conn[1], conn[2], conn[3]
    action[out["term"], 0] = 2
    flags[out["invalid"]] |= 1
    flags[add[0][out["needs_reset"]]] |= 2
    return action, flags


# ---- the stub model of golden_grow.npz ------------------------------------------------------------------------------

def config_dims(cfg):
    groups = [int(x) for x in cfg["groups"]]
    N, Fe = int(cfg["N"]), int(cfg["Fe"])
    dim_f_add = [N, *groups, Fe]
    return N, groups, Fe, dim_f_add, [N, Fe]


def stub_logits(cfg, r):
    """Round r's logits [B, W] (float32), regenerated from the seed: two live actions per graph, of a class (add bonded
    to node 0, add anywhere, connect, terminate) drawn per graph and round, and graph 0's terminate round."""
    N, groups, Fe, _, _ = config_dims(cfg)
    B, A = int(cfg["B"]), int(np.prod(groups)) * Fe
    W = N * A + N * Fe + 1
    rng = np.random.default_rng([int(cfg["stub_seed"]), r])
    z = rng.normal(size=(B, W)) * float(cfg["noise"])
    mode = rng.choice(4, size=B, p=[float(x) for x in cfg["mode_p"]])
    fav = np.zeros((B, W), bool)
    blocks = ((0, A), (0, N * A), (N * A, N * A + N * Fe), (W - 1, W))   # add bonded to node 0 (valid on a non-empty
    pick = rng.random((B, 2))                                        # graph), add anywhere, connect (on an empty
    for b in range(B):                                               # graph: from = -1), terminate
        lo, hi = blocks[mode[b]]
        e = lo + (pick[b] * (hi - lo)).astype(int)                   # two actions of the class per graph
        if int(cfg.get("last_group_zero", 0)) and mode[b] < 2:
            rem = e % A                                              # the last node-feature group's index -> 0
            e = e - rem + rem % Fe + (rem // Fe - (rem // Fe) % groups[-1]) * Fe
        fav[b, e] = True
    if int(cfg["graph0_terminate_round"]) == r:
        fav[0] = False
        fav[0, -1] = True
    # the rest of the row is pushed down far enough never to be drawn; with few live actions per row, few draws fall
    # within 1e-4 of a CDF boundary
    z = np.where(fav, z, z - float(cfg["drop"]))
    return z.astype(np.float32)


class StubModel(torch.nn.Module):
    """``gen.model`` of the golden runs: ignores the graphs, returns round k's ``stub_logits`` on the inputs' device."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg, self.calls = cfg, 0

    def forward(self, nodes, edges):
        z = stub_logits(self.cfg, self.calls)
        self.calls += 1
        return torch.from_numpy(z).to(nodes.device)


def run_oracle(cfg, max_rounds=4096):
    """The whole loop on CPU: stub logits -> torch's fp32 softmax (GraphGenerator.py:121) -> the pinned inverse-CDF draw
    (InverseCdfDraws) -> sampler_oracle.get_actions -> grow_round.  Returns (state, draws, coverage counts)."""
    N, groups, Fe, dim_f_add, dim_f_conn = config_dims(cfg)
    B = int(cfg["B"])
    s = new_state(B, N, sum(groups), Fe, 2 * N, 2 * B)
    draw = CO.InverseCdfDraws(int(cfg["draw_seed"]), B, max_rounds)
    cover = dict(graph0_terminate=0, add_to_full=0, connect_on_empty=0, duplicate_bond=0, term_and_invalid_round=0)
    while s["n"] < s["target"] and not s["error"]:
        apd = torch.softmax(torch.from_numpy(stub_logits(cfg, s["round"])), dim=1).numpy()
        out = SO.get_actions(apd, draw(apd), s["n_nodes"].astype(np.int64), s["edges"], dim_f_add, dim_f_conn)
        action, flags = actions_from_tuples(out, B, dim_f_add)
        nn = s["n_nodes"].astype(np.int64)
        kind = action[:, 0]
        cover["graph0_terminate"] += int(kind[0] == 2)
        cover["add_to_full"] += int(np.sum((kind == 0) & (nn >= N)))
        cover["connect_on_empty"] += int(np.sum((kind == 1) & (nn == 0)))
        conn = np.nonzero((kind == 1) & (nn > 0))[0]
        adj = s["edges"].sum(-1)
        cover["duplicate_bond"] += int(np.sum(adj[conn, action[conn, 1], action[conn, 3]] == 1))
        cover["term_and_invalid_round"] += int(np.any(kind[1:] == 2) and np.any(flags[1:] & 1))
        grow_round(s, action, out["likelihoods"].astype(np.float32), flags, groups, Fe)
        if s["error"]:
            break
    return s, draw, cover
