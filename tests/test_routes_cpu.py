"""CPU: the decoding route's golden and numpy model, the host-side helpers of graphinvent_amd.routes, and the
binding of the route entry points.  No device compute is issued.

The numpy model (tests/routes_model.py) is pinned twice: to the reference's own ``get_decoding_route_state`` output
(tests/golden/golden_routes.npz, written by tests/golden/make_golden_routes.py) and to the preprocessed files the
reference ships (gdb13_1K-debug_{train,valid}; the .npz copies hold the same bytes as the .h5)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import routes
from tests import routes_model as RM

GDB13_ADD, GDB13_CONN = [13, 5, 3, 3], [13, 3]


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "golden_routes.npz"))


def _fixture(golden_dir, split):
    d = np.load(os.path.join(golden_dir, f"gdb13_1K-debug_{split}.npz"))
    return d["nodes"], d["edges"], d["APDs"]


def test_golden_covers_what_it_should(golden_dir):
    G = _golden(golden_dir)
    assert list(G["configs"]) == ["gdb13", "arom5", "chiral6"]
    total = sum(G[f"{c}::mol_nodes"].shape[0] for c in G["configs"])
    assert total >= 130 and G["gdb13::mol_nodes"].shape[0] >= 136            # the 1 / 7 / 128 split exists
    assert len(G["arom5::dim_f_add"]) == 5 and len(G["chiral6::dim_f_add"]) == 6
    assert G["arom5::mol_edges"].shape[-1] == 4 and G["chiral6::mol_nodes"].shape[1] >= 40
    n_nodes = G["gdb13::mol_nodes"].any(axis=2).sum(axis=1)
    assert 1 in n_nodes and 2 in n_nodes and 13 in n_nodes
    # a last node whose bonds have mixed types, ending the type-major list on another node than index order would
    e = G["gdb13::mol_edges"]
    shows = 0
    for m in range(e.shape[0]):
        last = int(n_nodes[m]) - 1
        neigh = [(t, j) for t in range(3) for j in np.nonzero(e[m, :, last, t])[0]]
        shows += len(neigh) > 1 and neigh[-1][1] != max(j for _, j in neigh)
        assert len(neigh) <= 4
    assert shows >= 3
    degs = {int(e[m, :, int(n_nodes[m]) - 1].sum()) for m in range(e.shape[0])}
    assert {1, 2, 3, 4} <= degs


@pytest.mark.parametrize("config", ["gdb13", "arom5", "chiral6"])
def test_numpy_model_equals_the_reference_route(golden_dir, config):
    G = _golden(golden_dir)
    add, conn = G[f"{config}::dim_f_add"].tolist(), G[f"{config}::dim_f_conn"].tolist()
    rn, re, hot, rm, rs = RM.expand(G[f"{config}::mol_nodes"], G[f"{config}::mol_edges"], add, conn)
    assert np.array_equal(rn, G[f"{config}::rows_nodes"])
    assert np.array_equal(re, G[f"{config}::rows_edges"])
    assert np.array_equal(hot, G[f"{config}::hot"])
    assert np.array_equal(rm, G[f"{config}::row_mol"]) and np.array_equal(rs, G[f"{config}::row_step"])
    lengths = routes.route_lengths(G[f"{config}::mol_nodes"], G[f"{config}::mol_edges"])
    assert np.array_equal(lengths, np.bincount(rm))


@pytest.mark.parametrize("split, n_rows, n_expanded, first_route", [("train", 150, 151, 14), ("valid", 100, 131, 11)])
def test_numpy_model_against_the_shipped_preprocessed_files(golden_dir, split, n_rows, n_expanded, first_route):
    n, e, a = _fixture(golden_dir, split)
    assert n.shape[0] == n_rows
    mn, me = routes.molecules_from_rows(n, e, a, unique=True)
    assert mn.shape[0] == 10
    rn, re, hot, rm, rs = RM.expand(mn, me, GDB13_ADD, GDB13_CONN)
    assert rn.shape[0] == n_expanded
    have = {rn[r].tobytes() + re[r].tobytes() for r in range(rn.shape[0])}
    missing = [r for r in range(n_rows) if n[r].tobytes() + e[r].tobytes() not in have]
    assert missing == []                     # every row of the file, the all-zero-APD ones included
    # the route of the molecule at row 0 occupies rows 0 .. L-1 of the file, graph for graph
    assert np.array_equal(n[0], mn[0]) and np.array_equal(e[0], me[0])
    L0 = int(routes.route_lengths(mn[:1], me[:1])[0])
    assert L0 == first_route
    assert np.array_equal(n[:L0], rn[:L0]) and np.array_equal(e[:L0], re[:L0])
    # reported, not asserted: the file's APD sums against the merged expansion (the reference's group loop appends a
    # duplicate when a subgraph matches its group's last entry and cuts groups mid-molecule, which changes them)
    kn, ke, sums, _, _ = RM.merge(rn, re, hot, rm, rs, a.shape[1])
    at = {kn[r].tobytes() + ke[r].tobytes(): r for r in range(kn.shape[0])}
    live = [r for r in range(n_rows) if a[r].any()]
    agree = sum(np.array_equal(a[r], sums[at[n[r].tobytes() + e[r].tobytes()]]) for r in live)
    print(f"\n{split}: {agree} of {len(live)} APD sums of the file equal the merged expansion's")


def test_route_lengths_and_molecules_from_rows(golden_dir):
    n, e, a = _fixture(golden_dir, "train")
    mn, me = routes.molecules_from_rows(n, e, a)
    assert mn.dtype == np.int8 and mn.shape[1:] == (13, 8) and me.shape[1:] == (13, 13, 3)
    assert np.array_equal(mn, n[a[:, -1] > 0])
    un, ue = routes.molecules_from_rows(n, e, a, unique=True)
    keys = [un[i].tobytes() + ue[i].tobytes() for i in range(un.shape[0])]
    assert len(set(keys)) == len(keys) == 10 and mn.shape[0] >= 10
    lengths = routes.route_lengths(un, ue)
    assert lengths.dtype == np.int64 and lengths.tolist() == (ue.reshape(10, -1).sum(1) // 2 + 2).tolist()
    assert int(lengths.sum()) == 151 and 11 <= lengths.min() and lengths.max() <= 16
    tn, te = routes.molecules_from_rows(torch.from_numpy(n), torch.from_numpy(e), torch.from_numpy(a), unique=True)
    assert torch.is_tensor(tn) and np.array_equal(tn.numpy(), un) and np.array_equal(te.numpy(), ue)
    assert np.array_equal(routes.route_lengths(tn, te), lengths)
    with pytest.raises(ValueError):
        routes.route_lengths(un, ue[:, :, :5])


def test_batches_pack_to_the_row_budget_and_ranks_partition():
    rng = np.random.default_rng(0)
    lengths = rng.integers(2, 17, size=101)
    one = routes.plan_batches(lengths, 64, seed=3, epoch=2)
    order = np.random.default_rng([3, 2]).permutation(101)
    assert np.array_equal(np.concatenate(one), order)
    for b, nxt in zip(one, one[1:]):                          # greedy: the next molecule would not have fitted
        assert lengths[b].sum() <= 64 < lengths[b].sum() + lengths[nxt[0]]
    two = [routes.plan_batches(lengths, 64, rank=r, world_size=2, seed=3, epoch=2) for r in range(2)]
    assert len(two[0]) == len(two[1])                         # lock-step
    assert all(len(x) == len(y) for x, y in zip(*two))
    assert all(lengths[b].sum() <= 64 for t in two for b in t)
    seen = np.concatenate(two[0] + two[1])
    assert len(set(seen.tolist())) == len(seen) == 100        # disjoint; the odd molecule out is left
    other = routes.plan_batches(lengths, 64, seed=3, epoch=3)
    assert not np.array_equal(np.concatenate(other), order)
    assert np.array_equal(np.concatenate(routes.plan_batches(lengths, 64, shuffle=False)), np.arange(101))


def test_route_symbols_structs_and_abi_version(tmp_path):
    lib = L.load()
    for name in ("gi_route_plan_ws_bytes", "gi_route_rows_ws_bytes", "gi_route_plan", "gi_route_expand",
                 "gi_route_merge"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.gi_abi_version() == L.ABI_VERSION == 18       # the additions are additive
    d = routes._route_dims(10, 13, 8, 3, GDB13_ADD, GDB13_CONN)
    assert d.apd_width == 625 and list(d.seg)[:2] == [5, 3] and d.n_seg == 2
    plan = lib.gi_route_plan_ws_bytes(C.byref(d))
    assert plan >= 10 * (13 * 13 * 2 + 13 * 2 + 13 * 8) + 44 and plan % 16 == 0
    unmerged, merged = lib.gi_route_rows_ws_bytes(151, 0), lib.gi_route_rows_ws_bytes(151, 1)
    assert 151 * 12 <= unmerged < merged and merged % 16 == 0
    assert lib.gi_route_rows_ws_bytes(-1, 0) == -1
    d.apd_width = 624
    assert lib.gi_route_plan_ws_bytes(C.byref(d)) == -1      # GI_EINVAL: not the width of these dims
    d = routes._route_dims(1, 13, 8, 3, GDB13_ADD, GDB13_CONN)
    d.N = 200
    assert lib.gi_route_plan_ws_bytes(C.byref(d)) == -2      # GI_ELIMIT
    if shutil.which("gcc") is None:
        return
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "graphinvent_amd.h"', 'int main(void) {',
           '  printf("%zu %zu %zu %d %d\\n", sizeof(gi_route_dims), offsetof(gi_route_dims, seg), '
           'offsetof(gi_route_dims, apd_width), GI_ROUTE_COUNTS, GI_ABI_VERSION);',
           '  printf("%d %d %d %d %d %d %d\\n", GI_ROUTE_ERR_VALUE, GI_ROUTE_ERR_ONEHOT, GI_ROUTE_ERR_ASYMMETRIC, '
           'GI_ROUTE_ERR_MULTI_BOND, GI_ROUTE_ERR_CONNECT, GI_ROUTE_ERR_PADDING, GI_ROUTE_ERR_EMPTY);',
           '  return 0;', '}']
    cfile, exe = tmp_path / "route_sizes.c", tmp_path / "route_sizes"
    cfile.write_text("\n".join(src))
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, str(cfile), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(L.RouteDims), L.RouteDims.seg.offset,
                                                L.RouteDims.apd_width.offset, L.ROUTE_COUNTS, 18]
    assert [int(x) for x in out[1].split()] == [L.ROUTE_ERR_VALUE, L.ROUTE_ERR_ONEHOT, L.ROUTE_ERR_ASYMMETRIC,
                                                L.ROUTE_ERR_MULTI_BOND, L.ROUTE_ERR_CONNECT, L.ROUTE_ERR_PADDING,
                                                L.ROUTE_ERR_EMPTY]
    assert set(routes.ERROR_MESSAGES) == {1, 2, 4, 8, 16, 32, 64}


def test_python_boundary_raises_for_what_the_kernels_do_not_cover():
    n, e = torch.zeros(2, 13, 8, dtype=torch.int8), torch.zeros(2, 13, 13, 3, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU"):
        routes.expand(n, e, GDB13_ADD, GDB13_CONN)
    with pytest.raises(ValueError, match="GI_MAX_NODES"):
        routes._route_dims(1, 129, 8, 3, [129, 5, 3, 3], [129, 3])
    with pytest.raises(ValueError, match="GI_MAX_GROUPS"):
        routes._route_dims(1, 13, 8, 9, [13, 5, 3, 9], [13, 9])
    with pytest.raises(ValueError, match="dim_f_add"):
        routes._route_dims(1, 13, 8, 3, [13, 5, 4, 3], [13, 3])          # segments do not sum to Fn
    with pytest.raises(ValueError, match="dim_f_conn"):
        routes._route_dims(1, 13, 8, 3, GDB13_ADD, [13, 4])
    with pytest.raises(RuntimeError, match="no CPU"):
        routes.RouteLoader(n.numpy(), e.numpy(), GDB13_ADD, GDB13_CONN, 32, device="cpu")
    assert "symmetric" in routes.describe_errors(L.ROUTE_ERR_ASYMMETRIC | L.ROUTE_ERR_VALUE)
