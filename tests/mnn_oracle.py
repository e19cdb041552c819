"""
CPU restatement of the reference's ``MNN`` (gnn/mpnn.py:16-74 on ``SummationMPNN.forward``,
gnn/summation_mpnn.py:80-149), built from ``oracle.ggnn_oracle``'s ``gru_cell`` and ``global_readout`` so that the
SELU-branch pin and the dropout hook of that module apply unchanged.  Computes in ``nodes.dtype`` (fp32 or fp64).

  message of edge i <- j with bond vector e:  m = (sum_f e_f W[:, :, f]) h_j,  W = message_weights [M, H, Fe]
  messages summed into i; the GRU updates only nodes with at least one edge (as GGNN)
  graph_emb[b] = sum over ALL N slots of hidden[b] (isolated atoms included, padded slots add 0)
"""
from __future__ import annotations

import math
from collections import OrderedDict, namedtuple
from typing import Dict

import numpy as np
import torch

from oracle import ggnn_oracle as O

#: the fields an MNN ``constants`` namedtuple carries (parameters/defaults.py:145-169 + the derived dataset constants)
MNN_FIELDS = ("device", "n_node_features", "n_edge_features", "max_n_nodes", "len_f_add_per_node",
              "len_f_conn_per_node", "hidden_node_features", "message_size", "message_passes",
              "mlp1_depth", "mlp1_dropout_p", "mlp1_hidden_dim", "mlp2_depth", "mlp2_dropout_p", "mlp2_hidden_dim")

#: the reference's MNN hyper-parameter defaults (parameters/defaults.py:158-168)
MNN_DEFAULTS = dict(mlp1_depth=4, mlp1_dropout_p=0.0, mlp1_hidden_dim=500, mlp2_depth=4, mlp2_dropout_p=0.0,
                    mlp2_hidden_dim=500, hidden_node_features=100, message_passes=3, message_size=100)

#: small dims of golden_mnn_tiny.npz
TINY_MNN = dict(n_node_features=5, n_edge_features=3, max_n_nodes=6, len_f_add_per_node=18,
                len_f_conn_per_node=3, hidden_node_features=16, message_size=12, message_passes=2,
                mlp1_depth=2, mlp1_hidden_dim=32, mlp2_depth=2, mlp2_hidden_dim=36,
                mlp1_dropout_p=0.0, mlp2_dropout_p=0.0)


def mnn_config(n_atom_types: int, n_formal_charge: int, max_n_nodes: int, n_edge_features: int = 3,
               **overrides) -> dict:
    """MNN config (MNN fields only) for a dataset shape, reference defaults unless overridden."""
    cfg = dict(MNN_DEFAULTS, device="cpu", n_node_features=n_atom_types + n_formal_charge,
               n_edge_features=n_edge_features, max_n_nodes=max_n_nodes,
               len_f_add_per_node=n_atom_types * n_formal_charge * n_edge_features,
               len_f_conn_per_node=n_edge_features)
    cfg.update(overrides)
    unknown = set(cfg) - set(MNN_FIELDS)
    if unknown:
        raise KeyError(f"not an MNN field: {sorted(unknown)}")
    return cfg


def tiny_config(**overrides) -> dict:
    return dict(TINY_MNN, device="cpu", **overrides)


#: a namedtuple with exactly the MNN fields (no enn_*, gather_*, msg_*, att_*); module level, so that models built
#: from it pickle
MnnConstants = namedtuple("MnnConstants", MNN_FIELDS)


def as_constants(cfg: dict) -> MnnConstants:
    return MnnConstants(**{k: cfg[k] for k in MNN_FIELDS})


def param_shapes(cfg: dict) -> "OrderedDict[str, tuple]":
    """state_dict keys and shapes of the reference MNN in registration order (gnn/mpnn.py:21-53)."""
    H, M, Fe, N = cfg["hidden_node_features"], cfg["message_size"], cfg["n_edge_features"], cfg["max_n_nodes"]
    A, C = cfg["len_f_add_per_node"], cfg["len_f_conn_per_node"]
    items = [("message_weights", (M, H, Fe)), ("gru.weight_ih", (3 * H, M)), ("gru.weight_hh", (3 * H, H)),
             ("gru.bias_ih", (3 * H,)), ("gru.bias_hh", (3 * H,))]
    items += O._mlp_shapes("APDReadout.fAddNet1", H, cfg["mlp1_hidden_dim"], cfg["mlp1_depth"], A)
    items += O._mlp_shapes("APDReadout.fConnNet1", H, cfg["mlp1_hidden_dim"], cfg["mlp1_depth"], C)
    items += O._mlp_shapes("APDReadout.fAddNet2", N * A + H, cfg["mlp2_hidden_dim"], cfg["mlp2_depth"], N * A)
    items += O._mlp_shapes("APDReadout.fConnNet2", N * C + H, cfg["mlp2_hidden_dim"], cfg["mlp2_depth"], N * C)
    items += O._mlp_shapes("APDReadout.fTermNet2", H, cfg["mlp2_hidden_dim"], cfg["mlp2_depth"], 1)
    return OrderedDict(items)


def init_params(cfg: dict, seed: int = 0, dtype=torch.float32) -> "OrderedDict[str, torch.Tensor]":
    """Deterministic weights with the reference's init distributions, from numpy's PCG64 (machine independent):
    message_weights and GRU U(-1/sqrt(H), +), Linear weights Xavier-uniform, Linear biases U(-1/sqrt(fan_in), +)."""
    rng = np.random.default_rng(seed)
    H = cfg["hidden_node_features"]
    shapes = param_shapes(cfg)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for key, shape in shapes.items():
        if key.startswith("gru.") or key == "message_weights":
            bound = 1.0 / math.sqrt(H)
        elif key.endswith(".weight"):
            bound = math.sqrt(6.0 / (shape[0] + shape[1]))
        else:
            bound = 1.0 / math.sqrt(shapes[key[:-4] + "weight"][1])
        out[key] = torch.from_numpy(rng.uniform(-bound, bound, size=shape).astype(np.float32)).to(dtype)
    return out


def mnn_forward(P: Dict[str, torch.Tensor], cfg: dict, nodes: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """``MNN.forward``: nodes [B,N,Fn], edges [B,N,N,Fe] -> APD logits [B, N*A + N*Fe + 1]."""
    dtype = nodes.dtype
    H = cfg["hidden_node_features"]
    adjacency = edges.sum(dim=3)
    eb, ei, ej = adjacency.nonzero(as_tuple=True)
    nb, ni = adjacency.sum(-1).nonzero(as_tuple=True)
    summation = ((nb.view(-1, 1) == eb) & (ni.view(-1, 1) == ei)).to(dtype)
    evec = edges[eb, ei, ej, :]
    hidden = torch.zeros(nodes.shape[0], nodes.shape[1], H, dtype=dtype)
    hidden[:, :, :nodes.shape[2]] = nodes
    node_rows = hidden[nb, ni, :]
    W = P["message_weights"]
    for _ in range(cfg["message_passes"]):
        nghb = hidden[eb, ej, :]
        terms = torch.einsum("ef,mhf,eh->em", evec, W, nghb)                      # gnn/mpnn.py:58-63
        messages = summation @ terms
        node_rows = O.gru_cell(P, messages, node_rows)
        hidden = hidden.clone()
        hidden[nb, ni, :] = node_rows
    graph_emb = torch.sum(hidden, dim=1)                                           # gnn/mpnn.py:69-74
    return O.global_readout(P, hidden, graph_emb)


def typed_sums(h: np.ndarray, in_perm: np.ndarray, u_src: np.ndarray, u_type: np.ndarray,
               seg_off: np.ndarray, Fe: int) -> np.ndarray:
    """S[c, k * Fe + t] = sum over the dst-CSR slots of compact row c whose message row has type t of h[u_src, k]."""
    R, H = seg_off.size - 1, h.shape[1]
    S = np.zeros((R, H, Fe), dtype=h.dtype)
    for c in range(R):
        for s in range(seg_off[c], seg_off[c + 1]):
            u = in_perm[s]
            S[c, :, u_type[u]] += h[u_src[u]]
    return S.reshape(R, H * Fe)


def forward_backward(P, cfg, nodes, edges, target):
    """One forward + KL loss + backward; returns (logits, loss, grads-by-key), None for a parameter the forward never
    reads (message_weights and GRU at message_passes = 0), as the reference's ``.grad`` stays None."""
    leaves = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in P.items())
    out = mnn_forward(leaves, cfg, nodes, edges)
    loss = O.kl_loss(out, target)
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return out.detach(), loss.detach(), OrderedDict(zip(leaves.keys(), grads))


# ---- fp32 mirrors of the MNN kernels (csrc/gi_mnn.hip): the kernels only add, in a fixed documented order -----------
def u_types(g: dict) -> np.ndarray:
    """Bond type of every message row (rows are bond-type-major: type t = [type_off[t], type_off[t + 1]))."""
    return (np.searchsorted(g["type_off"], np.arange(g["U"]), side="right") - 1).astype(np.int64)


def typed_sums_mirror(h: np.ndarray, g: dict, Fe: int) -> np.ndarray:
    """``gi_typed_seg_sum`` in its own arithmetic: per type an fp32 accumulator that starts at 0 and takes the
    dst-CSR slots ``seg_off[c] .. seg_off[c + 1]`` of row c in ascending order.  h: fp32 [R, H] -> fp32 [R, H * Fe]."""
    assert h.dtype == np.float32
    R, H = g["seg_off"].size - 1, h.shape[1]
    ut = u_types(g)
    S = np.zeros((R, H, Fe), dtype=np.float32)
    for c in range(R):
        for s in range(g["seg_off"][c], g["seg_off"][c + 1]):
            u = g["in_perm"][s]
            S[c, :, ut[u]] = S[c, :, ut[u]] + h[g["u_src"][u]]
    return S.reshape(R, H * Fe)


def typed_sums_t_mirror(dS: np.ndarray, g: dict, Fe: int, dh0=None) -> np.ndarray:
    """``gi_typed_seg_sum_t`` in its own arithmetic: a zero fp32 accumulator takes, over the ``out_perm`` slots
    ``src_off[c] .. src_off[c + 1]`` of row c, each message row's edges ``mu_off[u] .. mu_off[u + 1]`` in ascending
    order; the result is ``dh0 + acc`` (accumulate) or ``acc``.  dS: fp32 [R, H * Fe] -> fp32 [R, H]."""
    assert dS.dtype == np.float32
    R = g["src_off"].size - 1
    H = dS.shape[1] // Fe
    d3 = dS.reshape(R, H, Fe)
    ut = u_types(g)
    acc = np.zeros((R, H), dtype=np.float32)
    for c in range(R):
        for s in range(g["src_off"][c], g["src_off"][c + 1]):
            u = g["out_perm"][s]
            for k in range(g["mu_off"][u], g["mu_off"][u + 1]):
                acc[c] = acc[c] + d3[g["mu_dst"][k], :, ut[u]]
    return acc if dh0 is None else (dh0.astype(np.float32) + acc)


def typed_sums_t(dS: np.ndarray, g: dict, Fe: int):
    """The transposed typed sum in dS.dtype (fp64 reference) with, per element, the number of terms and the sum of
    their magnitudes: (dh [R, H], terms [R], mag [R, H])."""
    R = g["src_off"].size - 1
    H = dS.shape[1] // Fe
    d3 = dS.reshape(R, H, Fe)
    ut = u_types(g)
    dh, mag, terms = np.zeros((R, H), dS.dtype), np.zeros((R, H), dS.dtype), np.zeros(R, np.int64)
    for c in range(R):
        for s in range(g["src_off"][c], g["src_off"][c + 1]):
            u = g["out_perm"][s]
            for k in range(g["mu_off"][u], g["mu_off"][u + 1]):
                x = d3[g["mu_dst"][k], :, ut[u]]
                dh[c] += x; mag[c] += np.abs(x); terms[c] += 1
    return dh, terms, mag


def typed_sums_bound(h: np.ndarray, g: dict, Fe: int) -> np.ndarray:
    """(terms - 1) * 2^-24 * sum |terms| per element of the typed sum [R, H * Fe] (fp64): what sequential fp32
    addition of `terms` numbers may lose."""
    ut = u_types(g)
    R, H = g["seg_off"].size - 1, h.shape[1]
    cnt = np.zeros((R, 1, Fe))
    for c in range(R):
        for s in range(g["seg_off"][c], g["seg_off"][c + 1]):
            cnt[c, 0, ut[g["in_perm"][s]]] += 1
    mag = typed_sums(np.abs(h.astype(np.float64)), g["in_perm"], g["u_src"], ut, g["seg_off"], Fe).reshape(R, H, Fe)
    return (np.maximum(cnt - 1, 0) * 2.0 ** -24 * mag).reshape(R, H * Fe)


def graph_sum_mirror(h: np.ndarray, cidx: np.ndarray, B: int, N: int) -> np.ndarray:
    """``gi_graph_sum_fwd`` in its own arithmetic: a zero fp32 accumulator takes the slots n = 0 .. N - 1."""
    assert h.dtype == np.float32
    acc = np.zeros((B, h.shape[1]), dtype=np.float32)
    c = np.asarray(cidx).reshape(B, N)
    for n in range(N):
        acc = acc + h[c[:, n]]
    return acc


def redraw_bond_types(e8: np.ndarray, rng) -> np.ndarray:
    """The same bonds with every bond's type drawn uniformly from 0 .. Fe - 1 (synthetic.make_batch gives the types
    beyond the third probability 0), written symmetrically."""
    Fe = e8.shape[3]
    out = np.zeros_like(e8)
    b, i, j = np.nonzero(np.triu(e8.any(3), 1))
    t = rng.integers(0, Fe, size=b.size)
    out[b, i, j, t] = 1
    out[b, j, i, t] = 1
    return out


def hub_graph(N: int, Fn: int, Fe: int, rng):
    """A star: node 0 bonded to the N - 1 others with mixed bond types (an (N - 1)-long destination segment and an
    (N - 1)-long source segment).  Returns int8 (nodes [N, Fn], edges [N, N, Fe])."""
    n = np.zeros((N, Fn), np.int8)
    n[np.arange(N), rng.integers(0, Fn, size=N)] = 1
    e = np.zeros((N, N, Fe), np.int8)
    t = np.arange(N - 1) % Fe
    rng.shuffle(t)
    e[0, np.arange(1, N), t] = 1
    e[np.arange(1, N), 0, t] = 1
    return n, e


#: kernel-test inputs by name -> hidden widths to run them at (13 and 50: a partial group of 4 columns; 1: below one)
KERNEL_CASES = dict({f"fe{k}": (13,) for k in range(1, 9)},
                    graphs=(1, 4, 13, 50), nodedup=(1, 4, 13, 50), no_edges=(13,), hub_in_batch=(13, 50),
                    hub_alone=(13,))


def kernel_case(name: str):
    """(nodes, edges, nodedup) of a kernel-test batch: one per bond-type count 1 .. 8 with uniformly drawn types
    (every template instantiation), the structural cases (a self-loop graph, a pair with two bond types, isolated
    atoms; with and without row sharing; no edges at all) and a 127-armed star at N = 128, inside a batch and alone."""
    from graphinvent_amd import synthetic
    if name.startswith("fe"):
        Fe = int(name[2:])
        n, e, _ = synthetic.make_batch(24, 9, 3, 2, Fe, seed=4 + Fe, frac_empty=0.1, frac_single=0.1)
        e = redraw_bond_types(e, np.random.default_rng(100 + Fe))
        assert e.any((0, 1, 2)).all()                          # every bond type occurs
        return n, e, False
    if name in ("graphs", "nodedup", "no_edges"):
        n, e, _ = synthetic.make_batch(24, 9, 3, 2, 3, seed=4, frac_empty=0.1, frac_single=0.1)
        n[0] = 0; e[0] = 0; n[0, 0, 0] = 1; n[0, 0, 3] = 1; e[0, 0, 0, 0] = 1    # dummy self-loop graph
        e[1, 0, 1, :] = 0; e[1, 0, 1, 0] = 1; e[1, 0, 1, 2] = 1                   # a pair with two bond types
        if name == "no_edges":
            e[:] = 0
        return n, e, name == "nodedup"
    if name in ("hub_in_batch", "hub_alone"):
        B = 6 if name == "hub_in_batch" else 1
        n, e, _ = synthetic.make_batch(B, 128, 3, 2, 3, seed=11, frac_empty=0.0, frac_single=0.0)
        n[0], e[0] = hub_graph(128, 5, 3, np.random.default_rng(12))
        return n, e, False
    raise KeyError(name)
