"""Golden node orders from the UNMODIFIED reference ``MolecularGraph.PreprocessingGraph``: ``breadth_first_search``,
``depth_first_search`` (MolecularGraph.py:328-433), ``reorder_nodes`` and ``pad_graph_representation`` (:592-633) —
the parts of ``node_remap`` (:435-461) that do not touch RDKit — and, for a subset, every
``get_decoding_route_state(k)`` of the reordered graph.

Runs only where the reference checkout is (``python tests/golden/make_golden_reorder.py [path/to/graphinvent]``), under
the stubs of ``make_golden_routes.py`` (its ``load_reference``), on that script's three configurations.  Every
odd-numbered molecule of a configuration gets a seeded permutation of its nodes first: the synthetic molecules are all
in a BFS-like order already, the permuted ones are not.  Graphs are bare ``PreprocessingGraph`` instances
(``object.__new__``, then ``constants``, ``n_nodes`` and the UNPADDED ``node_features`` / ``edge_features``).

For each molecule and each of K = 10 seeded rankings (a shuffle of 0..n-1, what ``node_remap`` draws with
``use_canon = False``) the start node is ``rank[0]``, as ``node_remap`` passes it.  Output ``golden_reorder.npz``, per
configuration ``c`` (cases are molecule-major, ranking-minor; orders and level sizes are padded with -1 / 0 to N):

  c::mol_nodes, c::mol_edges        the input molecules (int8, padded), c::dim_f_add, c::dim_f_conn
  c::case_mol, c::rank              the molecule of each case and its ranking
  c::bfs_order, c::dfs_order        what the two searches return
  c::bfs_levels                     sizes of the BFS levels (nodes at distance 0, 1, .. of the start node, from a
                                    distance computation of this script); the script asserts that they cut the
                                    reference's BFS order into exactly those distance classes
  c::bfs_nodes, c::bfs_edges,       ``reorder_nodes`` + ``pad_graph_representation`` under each of the two orders
  c::dfs_nodes, c::dfs_edges
  c::route_case, c::route_mode      the subset with recorded routes: case index and 0 (bfs) / 1 (dfs); DFS for the
  c::route_{rows_nodes,rows_edges,  first molecules' first two rankings, BFS for those of them with at most 8 nodes
     hot,row_graph,row_step}        (where the device's BFS order is the reference's); rows as in golden_routes.npz,
                                    row_graph indexing route_case
"""
import os
import random
import sys
import warnings
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_routes as R                                    # noqa: E402

K_RANKINGS = 10
ROUTE_MOLS = {"gdb13": 30, "arom5": 8, "chiral6": 4}             # molecules with recorded routes (2 rankings each)


def permuted(rng, nodes, edges):
    n = int(nodes.any(axis=1).sum())
    p = rng.permutation(n)
    out_n, out_e = np.zeros_like(nodes), np.zeros_like(edges)
    out_n[:n] = nodes[p]
    out_e[:n, :n] = edges[p][:, p]
    return out_n, out_e


def bare_graph(MG, constants, nodes, edges):
    g = object.__new__(MG.PreprocessingGraph)
    n = int(nodes.any(axis=1).sum())
    g.constants = constants
    g.n_nodes = n
    g.node_features = nodes[:n].astype(np.int32)
    g.edge_features = edges[:n, :n].astype(np.int32)
    return g


def distances(edges, n, start):
    adj = edges[:n, :n].any(axis=2)
    dist = np.full(n, -1)
    dist[start] = 0
    d = 0
    while (dist == d).any():
        reach = adj[dist == d].any(axis=0) & (dist < 0)
        d += 1
        dist[reach] = d
    assert (dist >= 0).all(), "disconnected molecule"
    return dist


def pad(seq, N, fill):
    out = np.full(N, fill, dtype=np.int8)
    out[:len(seq)] = seq
    return out


def record(MG, name, mols, N, seg, Fe):
    dim_f_add, dim_f_conn = [N] + list(seg) + [Fe], [N, Fe]
    Kc = namedtuple("K", "dim_f_add dim_f_conn n_edge_features max_n_nodes n_node_features")
    constants = Kc(dim_f_add, dim_f_conn, Fe, N, sum(seg))
    rng = np.random.default_rng({"gdb13": 31, "arom5": 32, "chiral6": 33}[name])
    mols = [permuted(rng, a, b) if m % 2 else (a, b) for m, (a, b) in enumerate(mols)]
    pyrng = random.Random(1234)
    rec = {k: [] for k in ("case_mol", "rank", "bfs_order", "dfs_order", "bfs_levels", "bfs_nodes", "bfs_edges",
                           "dfs_nodes", "dfs_edges", "route_case", "route_mode")}
    route_graphs = []
    for m, (nodes, edges) in enumerate(mols):
        n = int(nodes.any(axis=1).sum())
        for k in range(K_RANKINGS):
            ranking = list(range(n))
            pyrng.shuffle(ranking)                               # node_remap's `random.shuffle(atom_ranking)`
            case = len(rec["case_mol"])
            rec["case_mol"].append(m)
            rec["rank"].append(pad(ranking, N, -1))
            for mode, search in enumerate(("breadth_first_search", "depth_first_search")):
                g = bare_graph(MG, constants, nodes, edges)
                order = [int(x) for x in getattr(g, search)(node_ranking=ranking, node_init=ranking[0])]
                assert sorted(order) == list(range(n)), (name, m, k, search)
                g.node_ordering = order
                g.reorder_nodes()
                g.pad_graph_representation()
                rn, re = g.node_features.astype(np.int8), g.edge_features.astype(np.int8)
                tag = ("bfs", "dfs")[mode]
                rec[tag + "_order"].append(pad(order, N, -1))
                rec[tag + "_nodes"].append(rn)
                rec[tag + "_edges"].append(re)
                if mode == 0:
                    dist = distances(edges, n, ranking[0])
                    sizes = np.bincount(dist)
                    at = 0
                    for d, size in enumerate(sizes):              # the level-set property
                        assert set(order[at:at + size]) == set(np.nonzero(dist == d)[0].tolist()), (name, m, k, d)
                        at += size
                    rec["bfs_levels"].append(pad(sizes, N, 0))
                if m < ROUTE_MOLS[name] and k < 2 and (mode == 1 or n <= 8):
                    rec["route_case"].append(case)
                    rec["route_mode"].append(mode)
                    route_graphs.append((rn, re))
    out = {k: np.stack(v).astype(np.int8 if k not in ("case_mol", "route_case") else np.int32)
           for k, v in rec.items()}
    out.update(mol_nodes=np.stack([a for a, _ in mols]), mol_edges=np.stack([b for _, b in mols]),
               dim_f_add=np.array(dim_f_add), dim_f_conn=np.array(dim_f_conn))
    routes = R.record(MG, route_graphs, N, seg, Fe)
    out.update(route_rows_nodes=routes["rows_nodes"], route_rows_edges=routes["rows_edges"], route_hot=routes["hot"],
               route_row_graph=routes["row_mol"], route_row_step=routes["row_step"])
    return out


def main():
    warnings.simplefilter("ignore", DeprecationWarning)          # int() of a 1-element array, MolecularGraph.py:511-513
    MG, real_util = R.load_reference()
    configs = {"gdb13": R.gdb13_molecules(), "arom5": R.small_config(11, 20, 13, (4, 3, 4), 4),
               "chiral6": R.small_config(12, 12, 40, (3, 2, 3, 2), 4)}
    blob = {"configs": np.array(list(configs)), "util_is_the_references": np.array(real_util)}
    for name, (mols, N, seg, Fe) in configs.items():
        R.set_segments(seg, real_util)
        rec = record(MG, name, mols, N, seg, Fe)
        n = rec["mol_nodes"].any(axis=2).sum(axis=1)[rec["case_mol"]]
        same = (rec["bfs_order"] == rec["dfs_order"]).all(axis=1)
        print(f"{name}: {len(mols)} molecules, {len(n)} cases ({int((n <= 8).sum())} with n <= 8), "
              f"{len(rec['route_case'])} recorded routes ({len(rec['route_hot'])} rows), "
              f"BFS == DFS order in {int(same.sum())}")
        blob.update({f"{name}::{k}": v for k, v in rec.items()})
    out = os.path.join(R.HERE, "golden_reorder.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
