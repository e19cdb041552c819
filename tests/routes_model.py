"""Test helper: a numpy model of the decoding route and of the first-occurrence merge, written as the step-by-step
procedure (look at the last node, list its neighbours bond type first, take the last entry away), NOT as the closed
form the kernels use.  tests/test_routes_cpu.py pins it to the reference's own output (golden_routes.npz and the
shipped preprocessed fixtures); the GPU tests then use it where no golden exists (merged batches)."""
import numpy as np


def apd_width(dim_f_add, dim_f_conn):
    return int(np.prod(dim_f_add)) + int(np.prod(dim_f_conn)) + 1


def route(nodes, edges, dim_f_add, dim_f_conn):
    """[(nodes_k, edges_k, hot_k)] for k = 0 .. n_edges + 1 of one padded molecule (int8 arrays)."""
    nodes, edges = np.array(nodes, dtype=np.int8), np.array(edges, dtype=np.int8)
    seg, Fe = [int(s) for s in dim_f_add[1:-1]], int(dim_f_add[-1])
    bounds = np.concatenate([[0], np.cumsum(seg)])
    n_add = int(np.prod(dim_f_add))
    n = int(nodes.any(axis=1).sum())
    rows = [(nodes.copy(), edges.copy(), apd_width(dim_f_add, dim_f_conn) - 1)]
    while n > 0:
        last = n - 1
        feats = [int(np.argmax(nodes[last, bounds[s]:bounds[s + 1]])) for s in range(len(seg))]
        neigh = [(t, int(j)) for t in range(Fe) for j in np.nonzero(edges[:, last, t])[0]]
        if neigh:
            t, j = neigh[-1]
            if len(neigh) > 1:
                hot = n_add + j * Fe + t
            else:
                hot = int(np.ravel_multi_index([j] + feats + [t], dim_f_add))
                nodes[last] = 0
                n -= 1
            edges[j, last] = 0
            edges[last, j] = 0
        else:
            hot = int(np.ravel_multi_index([0] + feats + [0], dim_f_add))
            nodes[last] = 0
            n -= 1
        rows.append((nodes.copy(), edges.copy(), hot))
    return rows


def expand(mol_nodes, mol_edges, dim_f_add, dim_f_conn):
    """Unmerged rows of a batch: (nodes [R, N, Fn], edges [R, N, N, Fe], hot [R], row_mol [R], row_step [R])."""
    rn, re, hot, rm, rs = [], [], [], [], []
    for m in range(len(mol_nodes)):
        for k, (a, b, h) in enumerate(route(mol_nodes[m], mol_edges[m], dim_f_add, dim_f_conn)):
            rn.append(a); re.append(b); hot.append(h); rm.append(m); rs.append(k)
    N, Fn = mol_nodes.shape[1:]
    Fe = mol_edges.shape[3]
    return (np.array(rn, dtype=np.int8).reshape(-1, N, Fn), np.array(re, dtype=np.int8).reshape(-1, N, N, Fe),
            np.array(hot, dtype=np.int64), np.array(rm, dtype=np.int32), np.array(rs, dtype=np.int32))


def one_hot(hot, width, dtype=np.int64):
    out = np.zeros((len(hot), width), dtype=dtype)
    out[np.arange(len(hot)), hot] = 1
    return out


def merge(rn, re, hot, rm, rs, width):
    """First-occurrence merge of byte-identical (nodes, edges): kept rows in order, APD sums (int64)."""
    first, keep, sums = {}, [], []
    for r in range(len(rn)):
        key = rn[r].tobytes() + re[r].tobytes()
        at = first.get(key)
        if at is None:
            at = first[key] = len(keep)
            keep.append(r)
            sums.append(np.zeros(width, dtype=np.int64))
        sums[at][hot[r]] += 1
    keep = np.array(keep, dtype=np.int64)
    return rn[keep], re[keep], np.array(sums).reshape(-1, width), rm[keep], rs[keep]
