"""CPU: the node reordering's golden and numpy model, the device-drawn ranking's numpy mirror, and the binding and
Python boundary of graphinvent_amd.routes.reorder.  No device compute is issued.

The numpy model (tests/reorder_model.py) is pinned to the reference's own ``breadth_first_search``,
``depth_first_search`` and ``reorder_nodes`` output (tests/golden/golden_reorder.npz, written by
tests/golden/make_golden_reorder.py): DFS case for case; BFS by its level sets everywhere and exactly for molecules of
up to 8 nodes, where CPython's set order is ascending index (see the model's docstring)."""
import os
import re

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import routes
from tests import reorder_model as OM

CONFIGS = ["gdb13", "arom5", "chiral6"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(golden_dir, config):
    G = np.load(os.path.join(golden_dir, "golden_reorder.npz"))
    return {k.split("::", 1)[1]: G[k] for k in G.files if k.startswith(config + "::")}


def _cases(g):
    """(case, molecule nodes, edges, n, rank[:n]) of every case of a configuration."""
    n_of = g["mol_nodes"].any(axis=2).sum(axis=1)
    for c, m in enumerate(g["case_mol"]):
        n = int(n_of[m])
        yield c, g["mol_nodes"][m], g["mol_edges"][m], n, g["rank"][c, :n].astype(np.int64)


def test_golden_covers_what_it_should(golden_dir):
    G = np.load(os.path.join(golden_dir, "golden_reorder.npz"))
    assert list(G["configs"]) == CONFIGS
    for config, mols, N in (("gdb13", 140, 13), ("arom5", 20, 13), ("chiral6", 12, 40)):
        g = _golden(golden_dir, config)
        assert g["mol_nodes"].shape[:2] == (mols, N) and len(g["case_mol"]) == 10 * mols
        n_of = g["mol_nodes"].any(axis=2).sum(axis=1)
        for c, _, _, n, rank in _cases(g):
            assert sorted(rank.tolist()) == list(range(n)) and (g["rank"][c, n:] == -1).all()
        # input orders that are NOT BFS-like: a node i > 0 without a neighbour of lower index
        adj = g["mol_edges"].any(axis=3)
        unordered = sum(any(not adj[m, i, :i].any() for i in range(1, int(n_of[m]))) for m in range(mols))
        assert unordered >= mols // 5, (config, unordered)
        assert len(g["route_case"]) >= 10 and set(g["route_mode"].tolist()) == {0, 1}
        assert (g["bfs_order"] != g["dfs_order"]).any(axis=1).sum() >= len(g["case_mol"]) // 2


@pytest.mark.parametrize("config", CONFIGS)
def test_dfs_model_equals_the_reference_in_every_case(golden_dir, config):
    g = _golden(golden_dir, config)
    for c, _, edges, n, rank in _cases(g):
        assert OM.dfs(edges, n, rank) == g["dfs_order"][c, :n].tolist(), (config, c)
        assert (g["dfs_order"][c, n:] == -1).all()


@pytest.mark.parametrize("config", CONFIGS)
def test_bfs_model_has_the_reference_level_sets_and_its_order_up_to_8_nodes(golden_dir, config):
    g = _golden(golden_dir, config)
    total = exact = 0
    for c, _, edges, n, rank in _cases(g):
        ref, got = g["bfs_order"][c, :n].tolist(), OM.bfs(edges, n, rank)
        sizes = [int(s) for s in g["bfs_levels"][c] if s > 0]
        assert sum(sizes) == n and len(got) == n and got[0] == ref[0] == rank[0]
        at = 0
        for size in sizes:                               # the reference's level sizes cut both into the same sets
            level = got[at:at + size]
            assert set(level) == set(ref[at:at + size]), (config, c)
            assert level == sorted(level), (config, c)
            at += size
        total += 1
        if n <= 8:
            exact += 1
            assert got == ref, (config, c)
    print(f"\n{config}: {exact} of {total} BFS cases have n <= 8 and are exact")
    if config == "chiral6":
        assert exact >= 20
    else:
        assert 3 * exact >= total                         # the exact check is not hollow


@pytest.mark.parametrize("config", CONFIGS)
def test_reorder_model_equals_the_reference_reorder_nodes(golden_dir, config):
    g = _golden(golden_dir, config)
    for c, nodes, edges, n, _ in _cases(g):
        for tag in ("bfs", "dfs"):
            rn, re = OM.apply_order(nodes, edges, g[tag + "_order"][c, :n])
            assert np.array_equal(rn, g[tag + "_nodes"][c]) and np.array_equal(re, g[tag + "_edges"][c]), (config, c)
    # the batch form with the golden's rankings, DFS: orders and graphs at once
    pick = np.arange(0, len(g["case_mol"]), 7)
    mn, me = g["mol_nodes"][g["case_mol"][pick]], g["mol_edges"][g["case_mol"][pick]]
    rn, re, order = OM.reorder(mn, me, "dfs", rank=g["rank"][pick])
    assert np.array_equal(order, g["dfs_order"][pick]) and order.dtype == np.int32
    assert np.array_equal(rn, g["dfs_nodes"][pick]) and np.array_equal(re, g["dfs_edges"][pick])


def test_every_model_order_satisfies_the_expansion_contract(golden_dir):
    g = _golden(golden_dir, "gdb13")
    for c, nodes, edges, n, rank in _cases(g):
        for route in ("bfs", "dfs"):
            _, re = OM.apply_order(nodes, edges, OM.search(edges, n, rank, route))
            adj = re.any(axis=2)
            assert all(adj[i, :i].any() for i in range(1, n)), (c, route)


def test_mix64_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0 and with 1234567 (Vigna's reference implementation): the state
    # advances by the golden-ratio constant and mix64 adds it once more itself
    assert OM.mix64(0) == 0xE220A8397B1DCDAF
    assert OM.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert OM.mix64(1234567) == 6457827717110365317


def test_drawn_ranking_is_a_permutation_that_moves_with_the_epoch_not_with_the_batch(golden_dir):
    for n in (1, 2, 7, 13, 128):
        r = OM.drawn_rank(n, seed=3, epoch=0, mol_id=11)
        assert r.dtype == np.int32 and sorted(r.tolist()) == list(range(n))
    a, b = OM.drawn_rank(13, 3, 0, 11), OM.drawn_rank(13, 3, 1, 11)
    assert not np.array_equal(a, b)                                       # epochs differ
    assert not np.array_equal(a, OM.drawn_rank(13, 4, 0, 11))             # seeds differ
    assert not np.array_equal(a, OM.drawn_rank(13, 3, 0, 12))             # molecules differ
    assert np.array_equal(a[:0], a[:0]) and np.array_equal(a, OM.drawn_rank(13, 3, 0, 11))
    # a molecule's order depends on its dataset index, not on where it sits in a batch
    g = _golden(golden_dir, "gdb13")
    mn, me = g["mol_nodes"][:12], g["mol_edges"][:12]
    ids = np.arange(100, 112)
    perm = np.random.default_rng(0).permutation(12)
    for route in ("bfs", "dfs"):
        one = OM.reorder(mn, me, route, seed=5, epoch=2, mol_ids=ids)
        two = OM.reorder(mn[perm], me[perm], route, seed=5, epoch=2, mol_ids=ids[perm])
        assert all(np.array_equal(x[perm], y) for x, y in zip(one, two))
        assert not np.array_equal(one[2], OM.reorder(mn, me, route, seed=5, epoch=3, mol_ids=ids)[2])
    # default ids are the batch positions
    assert np.array_equal(OM.reorder(mn, me, "dfs", seed=5)[2], OM.reorder(mn, me, "dfs", seed=5, mol_ids=range(12))[2])


def test_reorder_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    assert re.search(r"^int\s+gi_route_reorder\s*\(", hdr, flags=re.M)
    assert re.search(r"#define\s+GI_ROUTE_ERR_RANK\s+128\b", hdr) and re.search(r"#define\s+GI_ROUTE_BFS\s+0\b", hdr)
    assert re.search(r"#define\s+GI_ROUTE_DFS\s+1\b", hdr)
    lib = L.load()
    assert "gi_route_reorder" in L.SIGNATURES and hasattr(lib, "gi_route_reorder")
    assert len(L.SIGNATURES["gi_route_reorder"][1]) == 16
    assert (L.ROUTE_ERR_RANK, L.ROUTE_BFS, L.ROUTE_DFS) == (128, 0, 1)
    assert lib.gi_abi_version() == L.ABI_VERSION == 18                    # an added entry point is compatible
    # argument checks that need no device: nothing is launched for any of these
    call = lambda M, N, Fn, Fe, mode: lib.gi_route_reorder(M, N, Fn, Fe, None, None, None, 0, 0, None, mode, None,
                                                           None, None, None, None)
    assert call(0, 13, 8, 3, L.ROUTE_BFS) == 0                             # an empty batch
    assert call(1, 13, 8, 3, L.ROUTE_DFS) == -1                            # GI_EINVAL: no buffers
    assert call(0, 13, 8, 3, 2) == -1                                      # unknown mode
    assert call(0, 0, 8, 3, 0) == -1
    assert call(0, 129, 8, 3, 0) == -2 and call(0, 13, 8, 9, 0) == -2      # GI_ELIMIT
    assert set(routes.REORDER_ERROR_MESSAGES) == {128}
    assert "permutation" in routes.describe_errors(L.ROUTE_ERR_RANK | L.ROUTE_ERR_VALUE)
    assert "not 0 or 1" in routes.describe_errors(L.ROUTE_ERR_RANK | L.ROUTE_ERR_VALUE)


def test_python_boundary_of_reorder_raises_like_expand():
    n, e = torch.zeros(2, 13, 8, dtype=torch.int8), torch.zeros(2, 13, 13, 3, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU"):
        routes.reorder(n, e)
    with pytest.raises(TypeError, match="tensors"):
        routes.reorder(n.numpy(), e.numpy())
    with pytest.raises((RuntimeError, TypeError)):                        # host tensors are refused whatever else
        routes.reorder(n.float(), e)
    with pytest.raises((RuntimeError, ValueError)):
        routes.reorder(n, e[:, :12])
    with pytest.raises(ValueError, match="route"):
        routes.reorder(n, e, route="canonical")
    with pytest.raises(ValueError, match="invalid"):
        routes.reorder(n, e, invalid="ignore")
    with pytest.raises(RuntimeError, match="no CPU"):
        routes.RouteLoader(n.numpy(), e.numpy(), [13, 5, 3, 3], [13, 3], 32, device="cpu", reorder="dfs")
    with pytest.raises(ValueError, match="reorder"):
        routes.RouteLoader(n.numpy(), e.numpy(), [13, 5, 3, 3], [13, 3], 32, reorder="canonical")
    if not torch.cuda.is_available():
        return
    dn, de = n.cuda(), e.cuda()                                           # raised before anything is launched
    with pytest.raises(TypeError, match="int8"):
        routes.reorder(dn.float(), de)
    with pytest.raises(ValueError, match="does not match"):
        routes.reorder(dn, de[:, :12])
    with pytest.raises(ValueError, match="rank"):
        routes.reorder(dn, de, rank=np.zeros((2, 12), dtype=np.int32))
    with pytest.raises(ValueError, match="mol_ids"):
        routes.reorder(dn, de, mol_ids=[1, 2, 3])
