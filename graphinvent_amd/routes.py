"""
Decoding routes on the device: from whole molecules to training rows.

The reference's preprocessing (``DataProcesser.get_subgraphs``, DataProcesser.py:167-271) writes one HDF row
(``nodes``, ``edges``, ``APDs``) for every subgraph on the decoding route of every molecule, about 15 rows per
GDB-13 molecule, and training streams those rows from disk over PCIe.  Here the molecules themselves are the
dataset: ``expand`` turns a batch of them into exactly those rows with the HIP kernels of ``csrc/gi_route.hip``,
and ``RouteLoader`` feeds a training loop from int8 molecules in pinned host memory.

A molecule is what ``PreprocessingGraph`` holds after ``node_remap`` and ``pad_graph_representation``
(MolecularGraph.py:435-461, 616-633): ``nodes[N, Fn]`` and ``edges[N, N, Fe]``, int8, 0 / 1, nodes in the
reference's (BFS / DFS) order so that every node i > 0 has a neighbour of lower index, zero padded; every node row
one-hot per feature segment, ``edges`` symmetric with at most one bond type per pair.

``reorder`` is ``node_remap`` itself, minus the source of the ranking: from a node ranking (given, or drawn on the
device per molecule and epoch) it runs the reference's breadth- or depth-first search and ``reorder_nodes`` with the
HIP kernel of ``csrc/gi_reorder.hip``, so molecules in ANY node order become valid input of ``expand``, and
``RouteLoader(reorder=...)`` trains on a different decoding route of every molecule in every epoch — the reference
draws one order per molecule at preprocessing time and keeps it.  Only SMILES parsing and RDKit's canonical ranking
(``use_canon``; pass it as ``rank``) stay outside; everything after them is here.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L

ERROR_MESSAGES = {
    L.ROUTE_ERR_VALUE: "an entry of nodes or edges is not 0 or 1",
    L.ROUTE_ERR_ONEHOT: "a node's feature row is not one-hot in every segment (atom type, formal charge, ...)",
    L.ROUTE_ERR_ASYMMETRIC: "edges is not symmetric (edges[i, j] != edges[j, i])",
    L.ROUTE_ERR_MULTI_BOND: "an atom pair carries several bond types",
    L.ROUTE_ERR_CONNECT: "a node i > 0 has no neighbour of lower index (nodes are not in a BFS / DFS order)",
    L.ROUTE_ERR_PADDING: "nodes are not a zero-padded prefix, or a bond touches a padding node or the diagonal",
    L.ROUTE_ERR_EMPTY: "a molecule has no node",
}


#: bits only ``reorder`` sets, next to those of ERROR_MESSAGES it shares (there ROUTE_ERR_CONNECT means: not connected)
REORDER_ERROR_MESSAGES = {
    L.ROUTE_ERR_RANK: "a row of rank is not a permutation of 0 .. n_nodes - 1",
}
_ROUTES = {"bfs": L.ROUTE_BFS, "dfs": L.ROUTE_DFS}


def describe_errors(bits: int) -> str:
    return "; ".join(msg for table in (ERROR_MESSAGES, REORDER_ERROR_MESSAGES) for bit, msg in table.items()
                     if bits & bit)


def _as_numpy(x) -> np.ndarray:
    if torch.is_tensor(x):
        if x.is_cuda:
            raise ValueError("host arrays expected (numpy or CPU tensors): this function does not touch the device")
        return x.numpy()
    return np.asarray(x)


def route_lengths(nodes, edges) -> np.ndarray:
    """Rows on the decoding route of each molecule, ``n_edges + 2`` (``get_decoding_route_length``,
    MolecularGraph.py:676-689), as an int64 array.  Takes numpy arrays or host tensors ``[M, N, Fn]`` /
    ``[M, N, N, Fe]`` and does not touch the device, so a loader can size its batches from it."""
    e = _as_numpy(edges)
    if e.ndim != 4 or e.shape[1] != e.shape[2]:
        raise ValueError(f"edges must be [M, N, N, Fe], got {e.shape}")
    n = _as_numpy(nodes)
    if n.ndim != 3 or n.shape[:2] != e.shape[:2]:
        raise ValueError(f"nodes {n.shape} does not match edges {e.shape}")
    return (e.reshape(e.shape[0], -1) != 0).sum(axis=1, dtype=np.int64) // 2 + 2


def molecules_from_rows(nodes, edges, apds, unique: bool = False):
    """The whole molecules of an existing preprocessed file: the rows whose ``f_term`` entry (the last of the flat
    APD) is positive, i.e. every route's row 0.  Returns ``(nodes, edges)`` of those rows in file order, numpy in,
    numpy out (host tensors likewise).  The reference's group loop writes a row twice when a subgraph matches the
    last entry of its group (DataProcesser.py:229), so a molecule can come back twice: ``unique=True`` keeps the
    first of byte-identical molecules."""
    as_tensor = torch.is_tensor(nodes)
    n, e, a = _as_numpy(nodes), _as_numpy(edges), _as_numpy(apds)
    if not (n.shape[0] == e.shape[0] == a.shape[0]):
        raise ValueError("nodes / edges / APDs disagree on the number of rows")
    idx = np.nonzero(a.reshape(a.shape[0], -1)[:, -1] > 0)[0]
    if unique:
        seen, keep = set(), []
        for i in idx:
            key = n[i].tobytes() + e[i].tobytes()
            if key not in seen:
                seen.add(key)
                keep.append(i)
        idx = np.asarray(keep, dtype=np.int64)
    out = (np.ascontiguousarray(n[idx]), np.ascontiguousarray(e[idx]))
    return tuple(torch.from_numpy(x) for x in out) if as_tensor else out


# ---- the device path ------------------------------------------------------------------------------------
def _route_dims(M: int, N: int, Fn: int, Fe: int, dim_f_add: Sequence[int], dim_f_conn: Sequence[int]) -> L.RouteDims:
    """gi_route_dims of a call; raises for what the kernels do not cover (as gnn.mpnn._check_limits does)."""
    dim_f_add, dim_f_conn = [int(x) for x in dim_f_add], [int(x) for x in dim_f_conn]
    if N > L.GI_MAX_NODES:
        raise ValueError(f"max_n_nodes = {N} exceeds the kernels' limit GI_MAX_NODES = {L.GI_MAX_NODES}")
    if Fe > L.GI_MAX_GROUPS:
        raise ValueError(f"n_edge_features = {Fe} exceeds the kernels' limit GI_MAX_GROUPS = {L.GI_MAX_GROUPS}")
    seg = dim_f_add[1:-1]
    if len(dim_f_add) < 3 or dim_f_add[0] != N or dim_f_add[-1] != Fe or not 1 <= len(seg) <= 4 or \
            any(s < 1 for s in seg) or sum(seg) != Fn:
        raise ValueError(f"dim_f_add = {dim_f_add} must be [N = {N}, feature segments summing to Fn = {Fn} "
                         f"(at most 4), Fe = {Fe}]")
    if dim_f_conn != [N, Fe]:
        raise ValueError(f"dim_f_conn = {dim_f_conn} must be [N, Fe] = {[N, Fe]}")
    width = int(np.prod(dim_f_add, dtype=np.int64)) + N * Fe + 1
    if width >= 2 ** 31 or int(np.prod(seg, dtype=np.int64)) > 2 ** 24:
        raise ValueError("APD width exceeds the kernels' 32-bit row index")
    d = L.RouteDims()
    d.M, d.N, d.Fn, d.Fe, d.n_seg, d.apd_width = M, N, Fn, Fe, len(seg), width
    for i, s in enumerate(seg):
        d.seg[i] = s
    return d


def _r16(x: int) -> int:
    return (x + 15) & ~15


class _Pending:
    """One enqueued expansion: device buffers and the counts still to be read back."""
    __slots__ = ("dims", "cap", "merge", "nodes", "edges", "apds", "row_mol", "row_step", "counts", "lengths",
                 "mol_err", "keep_alive", "hot")


def _check_inputs(nodes: torch.Tensor, edges: torch.Tensor):
    if not (torch.is_tensor(nodes) and torch.is_tensor(edges)):
        raise TypeError("nodes and edges must be torch tensors on the GPU")
    if not (nodes.is_cuda and edges.is_cuda):
        raise RuntimeError("nodes and edges must be CUDA (ROCm) tensors: the route kernels have no CPU fallback")
    if nodes.dtype != torch.int8 or edges.dtype != torch.int8:
        raise TypeError("nodes and edges must be int8 (the dtype of the preprocessed HDF)")
    if nodes.dim() != 3 or edges.dim() != 4 or edges.shape[:3] != (nodes.shape[0], nodes.shape[1], nodes.shape[1]):
        raise ValueError(f"edges shape {tuple(edges.shape)} does not match nodes {tuple(nodes.shape)}")
    if nodes.device != edges.device:
        raise ValueError("nodes and edges are on different devices")
    return nodes.contiguous(), edges.contiguous()


def _plan(nodes: torch.Tensor, edges: torch.Tensor, d: L.RouteDims):
    """Enqueue gi_route_plan on the current stream: (plan_ws, lengths, mol_err, counts), all on the device."""
    lib, dev = L.load(), nodes.device
    nbytes = lib.gi_route_plan_ws_bytes(C.byref(d))
    if nbytes < 0:
        L.check(int(nbytes), "gi_route_plan_ws_bytes")
    plan_ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
    lengths = torch.empty(d.M, dtype=torch.int32, device=dev)
    mol_err = torch.empty(d.M, dtype=torch.int32, device=dev)
    counts = torch.empty(L.ROUTE_COUNTS, dtype=torch.int32, device=dev)
    L.check(lib.gi_route_plan(C.byref(d), nodes.data_ptr(), edges.data_ptr(), plan_ws.data_ptr(),
                              lengths.data_ptr(), mol_err.data_ptr(), counts.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream), "gi_route_plan")
    return plan_ws, lengths, mol_err, counts


def _enqueue(nodes: torch.Tensor, edges: torch.Tensor, d: L.RouteDims, merge: bool, cap: int, planned=None,
             hash_mask: int = 2 ** 64 - 1, _apds: bool = True) -> _Pending:
    """Plan (unless `planned`), expand and merge on the current stream of the inputs' device, with no host wait.
    `cap` is the number of unmerged rows the outputs are sized for.  `_apds=False` (unmerged only; ``likelihood``'s)
    neither allocates nor writes the APD rows: `apds` is None and `hot` holds every row's hot APD index instead."""
    if merge and not _apds:
        raise ValueError("the merge sums APD rows: it cannot run without them")
    lib, dev = L.load(), nodes.device
    st = torch.cuda.current_stream(dev).cuda_stream
    plan_ws, lengths, mol_err, counts = planned if planned is not None else _plan(nodes, edges, d)
    N, Fn, Fe, W = d.N, d.Fn, d.Fe, d.apd_width
    f32 = d.M > 127                                           # a merged APD entry may reach M
    apd_dtype = L.DTYPE_F32 if f32 else L.DTYPE_I8

    def flat(row_bytes: int) -> torch.Tensor:
        return torch.empty(max(_r16(cap * row_bytes), 16), dtype=torch.int8, device=dev)

    def new_outputs(with_apd: bool):
        apd = None if not with_apd else \
            torch.empty(max(_r16(cap * W * 4) // 4, 4), dtype=torch.float32, device=dev) if f32 else flat(W)
        return (flat(N * Fn), flat(N * N * Fe), apd,
                torch.empty(max(cap, 1), dtype=torch.int32, device=dev),
                torch.empty(max(cap, 1), dtype=torch.int32, device=dev))

    nbytes = lib.gi_route_rows_ws_bytes(cap, 1 if merge else 0)
    if nbytes < 0:
        L.check(int(nbytes), "gi_route_rows_ws_bytes")
    rows_ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
    un, ue, ua, um, us = new_outputs(_apds)
    L.check(lib.gi_route_expand(C.byref(d), nodes.data_ptr(), plan_ws.data_ptr(), rows_ws.data_ptr(),
                                counts.data_ptr(), cap, hash_mask, un.data_ptr(), ue.data_ptr(),
                                None if merge or ua is None else ua.data_ptr(), apd_dtype, um.data_ptr(),
                                us.data_ptr(), st),
            "gi_route_expand")
    p = _Pending()
    p.dims, p.cap, p.merge, p.counts, p.lengths, p.mol_err = d, cap, merge, counts, lengths, mol_err
    p.hot = None
    if not _apds:
        ptr = C.c_void_p()
        L.check(lib.gi_route_rows_hot(rows_ws.data_ptr(), cap, C.byref(ptr)), "gi_route_rows_hot")
        at = int(ptr.value) - rows_ws.data_ptr()
        p.hot = rows_ws[at:at + 4 * max(cap, 1)].view(torch.int32)[:cap]
    if merge:
        on, oe, _, om, os_ = new_outputs(False)
        L.check(lib.gi_route_merge(C.byref(d), rows_ws.data_ptr(), counts.data_ptr(), cap, un.data_ptr(),
                                   ue.data_ptr(), um.data_ptr(), us.data_ptr(), on.data_ptr(), oe.data_ptr(),
                                   ua.data_ptr(), apd_dtype, om.data_ptr(), os_.data_ptr(), st), "gi_route_merge")
        un, ue, um, us = on, oe, om, os_
    p.nodes, p.edges, p.apds, p.row_mol, p.row_step = un, ue, ua, um, us
    p.keep_alive = (nodes, edges)
    return p


def _finish(p: _Pending, counts: Sequence[int], expect_rows: Optional[int], strict: bool = True):
    """Host side of an expansion once its counts are on the host: raise on error bits, cut the outputs to size."""
    err, total, merged = int(counts[0]), int(counts[1]), int(counts[2])
    if err and strict:
        raise ValueError("invalid molecule(s) in the batch: " + describe_errors(err))
    if total > p.cap or (expect_rows is not None and not err and total != expect_rows):
        raise ValueError(f"the molecules expand to {total} rows, not the {p.cap} the call was sized for "
                         "(n_rows must be route_lengths(nodes, edges).sum())")
    d, R = p.dims, merged if p.merge else total
    return (p.nodes[:R * d.N * d.Fn].view(R, d.N, d.Fn), p.edges[:R * d.N * d.N * d.Fe].view(R, d.N, d.N, d.Fe),
            p.apds[:R * d.apd_width].view(R, d.apd_width), p.row_mol[:R], p.row_step[:R])


def check(nodes: torch.Tensor, edges: torch.Tensor, dim_f_add: Sequence[int], dim_f_conn: Sequence[int]):
    """Per-molecule validity on the device: an int32 tensor ``[M]`` of error bits (``lib.ROUTE_ERR_*``, 0 = valid;
    ``describe_errors`` spells them out).  No read-back."""
    nodes, edges = _check_inputs(nodes, edges)
    M, N, Fn = nodes.shape
    d = _route_dims(M, N, Fn, edges.shape[3], dim_f_add, dim_f_conn)
    if M == 0:
        return torch.zeros(0, dtype=torch.int32, device=nodes.device)
    with torch.cuda.device(nodes.device):
        return _plan(nodes, edges, d)[2]


def expand(nodes: torch.Tensor, edges: torch.Tensor, dim_f_add: Sequence[int], dim_f_conn: Sequence[int], *,
           merge: bool = True, n_rows: Optional[int] = None, invalid: str = "raise", _hash_mask: int = 2 ** 64 - 1):
    """Training rows of ``M`` whole molecules, on the inputs' device and the current stream.

    Returns ``(nodes, edges, apds, row_mol, row_step)``.  For molecule ``m`` the rows are, in this order,
    ``get_decoding_route_state(k)`` for ``k = 0 .. n_edges + 1`` (MolecularGraph.py:691-732): ``k = 0`` is the whole
    molecule with the terminate-only APD, ``k >= 1`` has the APD computed before the k-th ``truncate_graph`` and the
    graph after it.  ``apds`` has the width of ``GGNN.forward``'s output (``f_add.ravel() | f_conn.ravel() | f_term``);
    it is int8 for ``M <= 127`` and fp32 above (a merged entry may reach ``M``), the two dtypes ``apd_kl_loss`` and
    the model read.  ``row_mol`` / ``row_step`` (int32) name the molecule and route index behind each row.

    ``merge=True`` (default): rows of the call whose ``nodes`` and ``edges`` are byte-identical become one row at the
    position of the first occurrence (molecule-major, route-index-minor), with the sum of their APDs, which is what
    DataProcesser.py:204-231 intends and ``Workflow.loss`` normalises away again (Workflow.py:854); ``row_mol`` /
    ``row_step`` then name that first occurrence.  Two accidents of the reference's Python loop are NOT reproduced:

    * its ``count == len(data_subgraphs)`` test (DataProcesser.py:229) appends a second copy of a subgraph that
      matches the last entry of the group;
    * it cuts a group off in the middle of a molecule at ``batch_size`` unique rows (:236-253) and drops the rest of
      that molecule's route.

    ``merge=False`` returns every row.

    Host synchronisation: the call ends with ONE read-back (error bits, row counts) — the merged row count is only
    known on the device.  ``n_rows`` = ``route_lengths(nodes, edges).sum()``, when the caller has it from the host
    copies, saves the second read-back that sizing the outputs otherwise needs.  (``RouteLoader`` takes both off the
    consumer's stream.)

    A molecule that violates the input contract raises ``ValueError`` naming the violated rule(s).  With
    ``invalid="skip"`` such molecules contribute no rows instead (``check`` tells which they are).
    """
    if invalid not in ("raise", "skip"):
        raise ValueError("invalid must be 'raise' or 'skip'")
    nodes, edges = _check_inputs(nodes, edges)
    M, N, Fn = nodes.shape
    Fe = edges.shape[3]
    d = _route_dims(M, N, Fn, Fe, dim_f_add, dim_f_conn)
    dev = nodes.device
    if M == 0:
        return (nodes.new_empty((0, N, Fn)), edges.new_empty((0, N, N, Fe)), nodes.new_empty((0, d.apd_width)),
                torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        planned = None
        if n_rows is None or invalid == "skip":
            planned = _plan(nodes, edges, d)
            head = planned[3].cpu().tolist()                 # read-back: sizes the outputs
            if head[0] and invalid == "raise":
                raise ValueError("invalid molecule(s) in the batch: " + describe_errors(head[0]))
            n_rows = head[1]
        p = _enqueue(nodes, edges, d, merge, int(n_rows), planned, _hash_mask)
        counts = p.counts.cpu().tolist()                     # read-back: error bits and the merged row count
    return _finish(p, counts, int(n_rows), strict=invalid == "raise")


def _enqueue_reorder(nodes: torch.Tensor, edges: torch.Tensor, route: str, rank: Optional[torch.Tensor], seed: int,
                     epoch: int, mol_ids: Optional[torch.Tensor], want_order: bool):
    """gi_route_reorder on the current stream of the inputs' device, with no host wait:
    (nodes', edges', order or None, mol_err).  `rank` int32 [M, N] and `mol_ids` int64 [M] are on that device."""
    lib, dev = L.load(), nodes.device
    M, N, Fn = nodes.shape
    Fe = edges.shape[3]
    out_n, out_e = torch.empty_like(nodes), torch.empty_like(edges)
    order = torch.empty((M, N), dtype=torch.int32, device=dev) if want_order else None
    mol_err = torch.empty(M, dtype=torch.int32, device=dev)
    L.check(lib.gi_route_reorder(M, N, Fn, Fe, nodes.data_ptr(), edges.data_ptr(),
                                 None if rank is None else rank.data_ptr(), int(seed) & (2 ** 64 - 1),
                                 int(epoch) & (2 ** 64 - 1), None if mol_ids is None else mol_ids.data_ptr(),
                                 _ROUTES[route], out_n.data_ptr(), out_e.data_ptr(),
                                 None if order is None else order.data_ptr(), mol_err.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream), "gi_route_reorder")
    return out_n, out_e, order, mol_err


def reorder(nodes: torch.Tensor, edges: torch.Tensor, *, route: str = "bfs", rank=None, seed: int = 0,
            epoch: int = 0, mol_ids=None, return_order: bool = False, invalid: str = "raise"):
    """``PreprocessingGraph.node_remap`` (MolecularGraph.py:435-461) for ``M`` molecules in one launch, on the inputs'
    device and the current stream: returns ``(nodes', edges')`` with ``nodes' = nodes[order]`` and ``edges' =
    edges[order][:, order]``, zero padded (``reorder_nodes``, ``pad_graph_representation``), where ``order`` is the
    reference's breadth- (``route="bfs"``) or depth-first (``"dfs"``) search from node ``rank[0]`` (the reference
    passes ``atom_ranking[0]``, a rank VALUE, as the start index; so does this).  The input nodes may be in any
    order; the output satisfies ``expand``'s contract.  ``return_order=True`` appends ``order`` (int32 ``[M, N]``: the
    input index of every output node, -1 past the molecule's nodes).

    ``rank`` (``[M, N]`` integers, tensor or array; the first ``n`` entries of a row count): a permutation of
    ``0 .. n-1`` per molecule, higher = more important — the reference's ``atom_ranking``, e.g. RDKit's canonical
    ranking.  ``rank=None`` draws it on the device, so nothing but the molecules crosses PCIe, as a pure function of
    ``(seed, epoch, mol_ids[m], node)`` (``mol_ids`` defaults to ``0 .. M-1``; give the molecules' indices in the
    dataset and a molecule's order in an epoch does not depend on batching, shuffling or the rank it lands on).

    ``"dfs"`` equals the reference's ``depth_first_search`` node for node.  ``"bfs"`` emits every level in ascending
    input index.  Its level sets are the reference's, but the reference appends a level as a Python ``set``
    (MolecularGraph.py:374), in CPython's hash-table order: that is ascending index while all ids are below the
    table size (8 slots for up to 4 elements), so the two agree for molecules of up to 8 nodes and differ inside
    levels for part of the larger ones.  CPython's probing sequence is NOT reproduced; every order produced is a
    valid BFS order.  As in the reference the ranking reaches a BFS through the start node only: ``"bfs"`` has at
    most ``n`` distinct orders per molecule, ``"dfs"`` many more.

    A molecule with an entry other than 0 / 1, nodes that are not a zero-padded prefix, asymmetric edges, no node,
    several connected components (the reference's loops never return on those) or a ``rank`` row that is not a
    permutation raises ``ValueError`` naming the rule, after ONE read-back of the error words.  ``invalid="skip"``
    reads nothing back: such molecules are copied through unchanged (``order`` = identity) and the per-molecule
    error bits (int32 ``[M]``, ``lib.ROUTE_ERR_*``) are appended to the result.
    """
    if invalid not in ("raise", "skip"):
        raise ValueError("invalid must be 'raise' or 'skip'")
    if route not in _ROUTES:
        raise ValueError("route must be 'bfs' or 'dfs'")
    nodes, edges = _check_inputs(nodes, edges)
    M, N, _ = nodes.shape
    if N > L.GI_MAX_NODES:
        raise ValueError(f"max_n_nodes = {N} exceeds the kernels' limit GI_MAX_NODES = {L.GI_MAX_NODES}")
    if edges.shape[3] > L.GI_MAX_GROUPS:
        raise ValueError(f"n_edge_features = {edges.shape[3]} exceeds the kernels' limit GI_MAX_GROUPS = "
                         f"{L.GI_MAX_GROUPS}")
    dev = nodes.device
    if rank is not None:
        rank = torch.as_tensor(rank)
        if tuple(rank.shape) != (M, N) or rank.dtype.is_floating_point:
            raise ValueError(f"rank must be integers of shape [M, N] = {[M, N]}, got {tuple(rank.shape)}")
        rank = rank.to(device=dev, dtype=torch.int32).contiguous()
    if mol_ids is not None:
        mol_ids = torch.as_tensor(mol_ids)
        if tuple(mol_ids.shape) != (M,) or mol_ids.dtype.is_floating_point:
            raise ValueError(f"mol_ids must be {M} integers, got shape {tuple(mol_ids.shape)}")
        mol_ids = mol_ids.to(device=dev, dtype=torch.int64).contiguous()
    with torch.cuda.device(dev):
        out_n, out_e, order, mol_err = _enqueue_reorder(nodes, edges, route, rank, seed, epoch, mol_ids, return_order)
        if invalid == "raise" and M:
            bits = int(np.bitwise_or.reduce(mol_err.cpu().numpy()))        # the read-back
            if bits:
                what = describe_errors(bits & ~L.ROUTE_ERR_CONNECT)
                if bits & L.ROUTE_ERR_CONNECT:
                    what = "; ".join(filter(None, [what, "a molecule is not connected"]))
                raise ValueError("invalid molecule(s) in the batch: " + what)
    out = (out_n, out_e) + ((order,) if return_order else ())
    return out + ((mol_err,) if invalid == "skip" else ())


def plan_batches(lengths: np.ndarray, batch_size: int, rank: int = 0, world_size: int = 1, seed: int = 0,
                 epoch: int = 0, shuffle: bool = True):
    """The molecule indices of every batch of an epoch on one rank (host arithmetic; see ``RouteLoader``)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    M, W = lengths.shape[0], world_size
    order = np.random.default_rng([seed, epoch]).permutation(M) if shuffle else np.arange(M)
    per = M // W                                              # molecules per rank; the remainder is left out
    if per == 0:
        return []
    shares = [order[(r + epoch) % W::W][:per] for r in range(W)]
    lens = np.stack([lengths[s] for s in shares])
    cuts, run = [0], np.zeros(W, dtype=np.int64)
    for i in range(per):
        if i > cuts[-1] and np.any(run + lens[:, i] > batch_size):
            cuts.append(i)
            run[:] = 0
        run += lens[:, i]
    cuts.append(per)
    return [shares[rank][a:b] for a, b in zip(cuts[:-1], cuts[1:])]


# ---- the loader -----------------------------------------------------------------------------------------
class RouteLoader:
    """Minibatches of training rows expanded on the device from whole molecules, with the iteration interface of
    ``loader.BlockStreamLoader`` (``len()``, ``set_epoch``, rank / world-size slicing): yields ``(nodes, edges, apds)``
    ready for ``model(nodes, edges)`` and ``apd_kl_loss``.

    * The molecules (int8 ``nodes [M, N, Fn]``, ``edges [M, N, N, Fe]``) stay in pinned host memory: one molecule
      per route instead of one row per route step crosses PCIe.
    * An epoch visits the molecules in a seeded order (``np.random.default_rng([seed, epoch]).permutation(M)``),
      identical on every rank; rank ``r`` takes every ``world_size``-th molecule of it starting at
      ``(r + epoch) % world_size``.  Consecutive molecules are packed into a batch until the next one would take the
      unmerged row count (``route_lengths``) past ``batch_size``.  With several ranks the cut points are the same on
      every rank (a batch ends where ANY rank's share would overflow), so all ranks yield the same number of
      batches — lock-step for the gradient all-reduce — from host arithmetic alone.
    * Batches have a varying number of rows (fewer than ``batch_size`` unmerged, fewer still after the merge); the
      model and the loss take ragged batches.
    * Pipelining: the copy and expansion of batch k + 2 are enqueued on the loader's side stream, and batch k + 1's
      merged row count is read back there and its compaction counts handed to ``ops.prefetch_compact``, while step k
      runs.  The consumer's stream only ever waits for an event of the side stream, never for the host.
    * ``reorder="bfs"`` / ``"dfs"`` (default ``None``: the molecules as stored): every batch goes through ``reorder``
      on the side stream between the copy and the expansion, with the ranking drawn on the device from the loader's
      ``seed``, the epoch and the molecule's index in the dataset.  Each epoch then trains on a different decoding
      route of every molecule, the same whatever the rank, world size or batch size, and the stored molecules may
      be in any node order.  Route lengths depend on the bond count only, so batches and row counts are unchanged;
      a molecule the reorder refuses (say, a disconnected one) is passed on unchanged and reported by the expansion.
    """

    def __init__(self, nodes, edges, dim_f_add: Sequence[int], dim_f_conn: Sequence[int], batch_size: int,
                 rank: int = 0, world_size: int = 1, seed: int = 0, shuffle: bool = True,
                 device: Optional[str] = "cuda", merge: bool = True, prefetch_compact: bool = True,
                 reorder: Optional[str] = None):
        if not 0 <= rank < world_size:
            raise ValueError("rank out of range")
        if reorder is not None and reorder not in _ROUTES:
            raise ValueError("reorder must be None, 'bfs' or 'dfs'")
        n, e = _as_numpy(nodes), _as_numpy(edges)
        if n.dtype != np.int8 or e.dtype != np.int8:
            raise TypeError("molecules are int8 arrays (the dtype of the preprocessed HDF)")
        self.lengths = route_lengths(n, e)
        self.n_molecules = n.shape[0]
        if self.n_molecules and int(self.lengths.max()) > batch_size:
            raise ValueError(f"a molecule's route has {int(self.lengths.max())} rows: batch_size = {batch_size} "
                             "cannot hold it")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RouteLoader expands on the GPU: the route kernels have no CPU fallback")
        self.dims = _route_dims(0, n.shape[1], n.shape[2], e.shape[3], dim_f_add, dim_f_conn)
        self._dim_f_add, self._dim_f_conn = list(dim_f_add), list(dim_f_conn)
        self.batch_size, self.rank, self.world, self.seed, self.shuffle = int(batch_size), rank, world_size, seed, shuffle
        self.merge, self.prefetch_compact, self.reorder = merge, prefetch_compact, reorder
        self.epoch = 0
        self._nodes = torch.from_numpy(np.ascontiguousarray(n)).pin_memory()
        self._edges = torch.from_numpy(np.ascontiguousarray(e)).pin_memory()
        self._stream = torch.cuda.Stream(self.device)
        self._stage, self._counts_host = None, None
        self._plan_cache = None
        self.pinned_bytes = self._nodes.numel() + self._edges.numel()
        self.rows_yielded = 0                                 # rows handed to the consumer so far (after the merge)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    # ---- epoch plan (host arithmetic only; the cut points are identical on every rank) --------------------
    def _epoch_plan(self):
        key = (self.epoch,)
        if self._plan_cache is None or self._plan_cache[0] != key:
            batches = plan_batches(self.lengths, self.batch_size, self.rank, self.world, self.seed, self.epoch,
                                   self.shuffle)
            self._plan_cache = (key, [(idx, int(self.lengths[idx].sum())) for idx in batches])
        return self._plan_cache[1]

    def __len__(self) -> int:
        return len(self._epoch_plan())

    def batch_molecules(self):
        """The molecule indices of every batch of the current epoch on this rank, in order."""
        return [idx.copy() for idx, _ in self._epoch_plan()]

    # ---- pipeline stages ----------------------------------------------------------------------------------
    def _launch(self, idx: np.ndarray, rows: int, slot: int, epoch: int = 0):
        """Gather the molecules into a pinned staging slot; copy, (reorder,) plan, expand and merge on the side
        stream."""
        k = idx.shape[0]
        if self._stage is None:
            cap = max(self.batch_size // 2, 1)                # a route has at least 2 rows
            mk = lambda t: torch.empty((cap,) + tuple(t.shape[1:]), dtype=torch.int8).pin_memory()
            self._stage = [(mk(self._nodes), mk(self._edges)) for _ in range(3)]
            self._counts_host = [torch.empty(L.ROUTE_COUNTS, dtype=torch.int32).pin_memory() for _ in range(3)]
            self.pinned_bytes += sum(a.numel() + b.numel() for a, b in self._stage)
            if self.reorder is not None:                      # the batch's dataset indices: the kernel's mol_ids
                self._stage_ids = [torch.empty(cap, dtype=torch.int64).pin_memory() for _ in range(3)]
                self.pinned_bytes += 3 * cap * 8
        sn, se = self._stage[slot]
        np.take(self._nodes.numpy().reshape(self.n_molecules, -1), idx, axis=0,
                out=sn.numpy().reshape(sn.shape[0], -1)[:k])
        np.take(self._edges.numpy().reshape(self.n_molecules, -1), idx, axis=0,
                out=se.numpy().reshape(se.shape[0], -1)[:k])
        d = _route_dims(k, self.dims.N, self.dims.Fn, self.dims.Fe, self._dim_f_add, self._dim_f_conn)
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            dn = sn[:k].to(self.device, non_blocking=True)
            de = se[:k].to(self.device, non_blocking=True)
            if self.reorder is not None:
                ids = self._stage_ids[slot]
                ids.numpy()[:k] = idx
                dn, de, _, _ = _enqueue_reorder(dn, de, self.reorder, None, self.seed, epoch,
                                                ids[:k].to(self.device, non_blocking=True), False)
            p = _enqueue(dn, de, d, self.merge, rows)
            host = self._counts_host[slot]
            host.copy_(p.counts, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        return p, host, ev, rows

    def _finalise(self, launched):
        """The merged row count is on the host once the side stream reaches the event (the HOST waits here, one
        batch ahead of the consumer); cut the outputs and start the compaction counts for them."""
        p, host, ev, rows = launched
        ev.synchronize()
        out = _finish(p, host.tolist(), rows)[:3]
        with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
            if self.prefetch_compact:
                from . import ops
                ops.prefetch_compact(out[0], out[1], stream=self._stream)
            done = torch.cuda.Event()
            done.record(self._stream)
        return out, done

    def _hand_over(self, ready, cur):
        out, done = ready
        cur.wait_event(done)                                  # the consumer's stream waits for ITS batch only
        for t in out:
            t.record_stream(cur)
        self.rows_yielded += out[0].shape[0]
        return out

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        batches, epoch = self._epoch_plan(), self.epoch
        cur = torch.cuda.current_stream(self.device)
        launched, ready = None, None
        for i, (idx, rows) in enumerate(batches):
            nxt = self._launch(idx, rows, i % 3, epoch)
            if launched is not None:
                fin = self._finalise(launched)
                if ready is not None:
                    yield self._hand_over(ready, cur)
                ready = fin
            launched = nxt
        if launched is not None:
            fin = self._finalise(launched)
            if ready is not None:
                yield self._hand_over(ready, cur)
            yield self._hand_over(fin, cur)
