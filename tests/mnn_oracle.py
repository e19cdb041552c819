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
