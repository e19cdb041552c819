"""GPU: graphinvent_amd.routes.reorder (csrc/gi_reorder.hip) against the reference's golden node orders and the numpy
model, byte for byte; the device-drawn ranking against its numpy mirror; reorder + expand against the reference's
``node_remap`` + ``get_decoding_route_state`` end to end; the input checks; RouteLoader(reorder=...)."""
import os
import warnings

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import routes
from tests import molio
from tests import reorder_model as OM
from tests import routes_model as RM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GDB13_ADD, GDB13_CONN = [13, 5, 3, 3], [13, 3]
CONFIGS = ["gdb13", "arom5", "chiral6"]


def _golden(golden_dir, config):
    G = np.load(os.path.join(golden_dir, "golden_reorder.npz"))
    g = {k.split("::", 1)[1]: G[k] for k in G.files if k.startswith(config + "::")}
    g["dim_f_add"], g["dim_f_conn"] = g["dim_f_add"].tolist(), g["dim_f_conn"].tolist()
    return g


def _fixture_molecules(golden_dir):
    ns, es = [], []
    for split in ("train", "valid"):
        d = np.load(os.path.join(golden_dir, f"gdb13_1K-debug_{split}.npz"))
        n, e = routes.molecules_from_rows(d["nodes"], d["edges"], d["APDs"], unique=True)
        ns.append(n); es.append(e)
    return np.concatenate(ns), np.concatenate(es)


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


def _assert_equals_model(out, model):
    n, e, order = _host(out)
    assert n.dtype == np.int8 and e.dtype == np.int8 and order.dtype == np.int32
    assert np.array_equal(order, model[2])
    assert np.array_equal(n, model[0])
    assert np.array_equal(e, model[1])


# ---- the kernel against the reference and the model --------------------------------------------------------
@pytest.mark.parametrize("route", ["bfs", "dfs"])
@pytest.mark.parametrize("config", CONFIGS)
def test_given_ranking_equals_the_reference_and_the_model(golden_dir, config, route):
    g = _golden(golden_dir, config)
    mn, me = g["mol_nodes"][g["case_mol"]], g["mol_edges"][g["case_mol"]]
    rank = g["rank"].astype(np.int32)
    out = routes.reorder(*_dev(mn, me), route=route, rank=torch.from_numpy(rank).to(DEV), return_order=True)
    _assert_equals_model(out, OM.reorder(mn, me, route, rank=rank))
    n, e, order = _host(out)
    if route == "dfs":                                       # the reference, case for case
        exact = np.ones(len(rank), dtype=bool)
    else:                                                    # the reference where CPython's set order is ascending
        exact = mn.any(axis=2).sum(axis=1) <= 8
        assert exact.sum() >= 20
        for c in range(len(rank)):                           # and its level sets everywhere
            at = 0
            for size in g["bfs_levels"][c]:
                assert set(order[c, at:at + size].tolist()) == set(g["bfs_order"][c, at:at + size].tolist())
                at += size
    assert np.array_equal(order[exact], g[route + "_order"][exact].astype(np.int32))
    assert np.array_equal(n[exact], g[route + "_nodes"][exact])
    assert np.array_equal(e[exact], g[route + "_edges"][exact])
    # the same ranking handed over as a host array, without the order
    short = routes.reorder(*_dev(mn[:5], me[:5]), route=route, rank=rank[:5])
    assert len(short) == 2 and np.array_equal(short[0].cpu().numpy(), n[:5])


@pytest.mark.parametrize("route", ["bfs", "dfs"])
@pytest.mark.parametrize("M, N, Fn, Fe", [(1, 13, 8, 3), (7, 13, 8, 3), (3000, 13, 8, 3), (257, 40, 10, 4),
                                          (48, 128, 5, 8), (33, 128, 3, 1), (100, 16, 16, 2)])
def test_random_batches_equal_the_model(M, N, Fn, Fe, route):
    """Single atoms, n == N, chains (deepest BFS, longest DFS branch), stars (widest level, a DFS that backtracks
    after every node) and ring systems in random input orders; N up to GI_MAX_NODES, Fe up to GI_MAX_GROUPS; row
    pitches that are and are not multiples of 16."""
    assert N <= L.GI_MAX_NODES and Fe <= L.GI_MAX_GROUPS
    rng = np.random.default_rng([M, N, Fe])
    mn, me, rank = OM.random_batch(rng, M, N, Fn, Fe)
    n_of = mn.any(axis=2).sum(axis=1)
    assert M < 7 or (1 in n_of and N in n_of)
    dn, de = _dev(mn, me)
    out = routes.reorder(dn, de, route=route, rank=rank, return_order=True)
    model = OM.reorder(mn, me, route, rank=rank)
    _assert_equals_model(out, model)
    again = routes.reorder(dn, de, route=route, rank=rank, return_order=True)        # two runs: identical bytes
    assert all(torch.equal(x, y) for x, y in zip(out, again))
    adj = model[1].any(axis=3)                                # expand's order rule holds for every output
    assert all(adj[m, i, :i].any() for m in range(min(M, 200)) for i in range(1, int(n_of[m])))


def test_unaligned_views_of_a_larger_buffer():
    """Molecule byte ranges that start at any address modulo 16: slices of a batch are views at odd offsets."""
    rng = np.random.default_rng(5)
    mn, me, rank = OM.random_batch(rng, 40, 13, 8, 3)         # pitches 104 and 507 bytes
    dn, de = _dev(mn, me)
    for lo in (1, 2, 3, 5):
        out = routes.reorder(dn[lo:lo + 9], de[lo:lo + 9], route="dfs", rank=rank[lo:lo + 9], return_order=True)
        want = OM.reorder(mn[lo:lo + 9], me[lo:lo + 9], "dfs", rank=rank[lo:lo + 9])
        _assert_equals_model(out, want)
        # the same molecules `lo` bytes into an allocation that holds 1 everywhere else: a read past either end of
        # the batch meets a set entry
        pn, pe = molio.to_dev(mn[lo:lo + 9], misalign=lo), molio.to_dev(me[lo:lo + 9], misalign=lo)
        _assert_equals_model(routes.reorder(pn, pe, route="dfs", rank=rank[lo:lo + 9], return_order=True), want)
        assert molio.padding_intact(pn) and molio.padding_intact(pe)


# ---- the device-drawn ranking ------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["bfs", "dfs"])
def test_drawn_ranking_equals_the_numpy_mirror(golden_dir, route):
    g = _golden(golden_dir, "gdb13")
    mn, me = g["mol_nodes"], g["mol_edges"]
    dn, de = _dev(mn, me)
    orders = []
    for seed, epoch in ((0, 0), (0, 1), (7, 0), (2 ** 63 + 5, 2 ** 40)):
        out = routes.reorder(dn, de, route=route, seed=seed, epoch=epoch, return_order=True)
        _assert_equals_model(out, OM.reorder(mn, me, route, seed=seed, epoch=epoch))
        orders.append(out[2].cpu().numpy())
    assert not np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[0], orders[2])
    # mol_ids: dataset indices, here far from the batch positions; as a tensor and as an array
    ids = np.arange(mn.shape[0], dtype=np.int64) * 1000003 + 17
    out = routes.reorder(dn, de, route=route, seed=3, epoch=4, mol_ids=torch.from_numpy(ids).to(DEV),
                         return_order=True)
    model = OM.reorder(mn, me, route, seed=3, epoch=4, mol_ids=ids)
    _assert_equals_model(out, model)
    assert not np.array_equal(model[2], OM.reorder(mn, me, route, seed=3, epoch=4)[2])
    # a batch permutation moves every molecule's result with it
    perm = np.random.default_rng(1).permutation(mn.shape[0])
    moved = routes.reorder(*_dev(mn[perm], me[perm]), route=route, seed=3, epoch=4, mol_ids=ids[perm],
                           return_order=True)
    assert all(np.array_equal(x[perm], y) for x, y in zip(_host(out), _host(moved)))


def test_drawn_ranking_at_128_nodes():
    rng = np.random.default_rng(9)
    mn, me, _ = OM.random_batch(rng, 20, 128, 4, 3)
    for route in ("bfs", "dfs"):
        out = routes.reorder(*_dev(mn, me), route=route, seed=11, epoch=2, return_order=True)
        _assert_equals_model(out, OM.reorder(mn, me, route, seed=11, epoch=2))


# ---- the reference end to end: node_remap, then get_decoding_route_state -----------------------------------
@pytest.mark.parametrize("config", CONFIGS)
def test_reorder_then_expand_equals_the_reference_routes_of_the_reordered_molecules(golden_dir, config):
    g = _golden(golden_dir, config)
    add, conn = g["dim_f_add"], g["dim_f_conn"]
    width = RM.apd_width(add, conn)
    for mode, route in enumerate(("bfs", "dfs")):
        graphs = np.nonzero(g["route_mode"] == mode)[0]
        assert len(graphs) >= 2
        cases = g["route_case"][graphs]
        mn, me = g["mol_nodes"][g["case_mol"][cases]], g["mol_edges"][g["case_mol"][cases]]
        rn, re = routes.reorder(*_dev(mn, me), route=route, rank=g["rank"][cases].astype(np.int32))
        n, e, a, rm, rs = _host(routes.expand(rn, re, add, conn, merge=False))
        rows = np.isin(g["route_row_graph"], graphs)
        assert np.array_equal(n, g["route_rows_nodes"][rows]) and np.array_equal(e, g["route_rows_edges"][rows])
        assert np.array_equal(a, RM.one_hot(g["route_hot"][rows], width, a.dtype))
        assert np.array_equal(rm, np.searchsorted(graphs, g["route_row_graph"][rows]))
        assert np.array_equal(rs, g["route_row_step"][rows])


# ---- invalid input -----------------------------------------------------------------------------------------
def _three(golden_dir):
    """Three connected gdb13 molecules of 5 .. 11 nodes (the middle one gets broken) and valid rankings."""
    g = _golden(golden_dir, "gdb13")
    n_of = g["mol_nodes"].any(axis=2).sum(axis=1)
    pick = np.nonzero((n_of >= 5) & (n_of <= 11))[0][[0, 3, 6]]
    mn, me = g["mol_nodes"][pick].copy(), g["mol_edges"][pick].copy()
    rank = np.stack([g["rank"][np.nonzero(g["case_mol"] == m)[0][0]] for m in pick]).astype(np.int32)
    return mn, me, rank, int(n_of[pick[1]])


def _break(kind, mn, me, rank, n):
    last = n - 1
    if kind == "not_zero_padded":
        mn[1, n + 1, 0] = 1                                               # a node behind a gap
        return L.ROUTE_ERR_PADDING, "zero-padded"
    if kind == "bond_on_padding":
        me[1, 0, n, 0] = me[1, n, 0, 0] = 1
        return L.ROUTE_ERR_PADDING, "padding node"
    if kind == "asymmetric":
        j, t = np.argwhere(me[1, last])[0]
        me[1, j, last, t] = 0
        return L.ROUTE_ERR_ASYMMETRIC, "symmetric"
    if kind == "asymmetric_type":                                         # same pair, another bond type one way
        j, t = np.argwhere(me[1, last])[0]
        me[1, j, last, t], me[1, j, last, (t + 1) % 3] = 0, 1
        return L.ROUTE_ERR_ASYMMETRIC, "symmetric"
    if kind == "value_2":
        j, t = np.argwhere(me[1, last])[0]
        me[1, last, j, t] = me[1, j, last, t] = 2
        return L.ROUTE_ERR_VALUE, "not 0 or 1"
    if kind == "node_value":
        mn[1, 0, np.argmax(mn[1, 0])] = -1
        return L.ROUTE_ERR_VALUE, "not 0 or 1"
    if kind == "disconnected":
        nb = np.nonzero(me[1, 0].any(axis=1))[0]                          # cut node 0 off
        me[1, 0] = 0
        me[1, :, 0] = 0
        assert len(nb) >= 1
        return L.ROUTE_ERR_CONNECT, "not connected"
    if kind == "rank_repeats":
        rank[1, 0] = rank[1, 1]
        return L.ROUTE_ERR_RANK, "permutation"
    if kind == "rank_out_of_range":
        rank[1, np.argmax(rank[1, :n])] = n
        return L.ROUTE_ERR_RANK, "permutation"
    raise KeyError(kind)


@pytest.mark.parametrize("route", ["bfs", "dfs"])
@pytest.mark.parametrize("kind", ["not_zero_padded", "bond_on_padding", "asymmetric", "asymmetric_type", "value_2",
                                  "node_value", "disconnected", "rank_repeats", "rank_out_of_range"])
def test_invalid_molecules_come_back_unchanged_with_their_bit(golden_dir, kind, route):
    """Every call here RETURNS: the kernel's loops are bounded by the dims whatever the data holds."""
    mn, me, rank, n = _three(golden_dir)
    good = OM.reorder(mn, me, route, rank=rank)
    bit, word = _break(kind, mn, me, rank, n)
    dn, de = _dev(mn, me)
    rn, re, order, err = routes.reorder(dn, de, route=route, rank=rank, return_order=True, invalid="skip")
    assert err.dtype == torch.int32 and err.cpu().tolist() == [0, bit, 0], (kind, err.cpu().tolist())
    rn, re, order = _host((rn, re, order))
    assert np.array_equal(rn[1], mn[1]) and np.array_equal(re[1], me[1])             # copied through
    assert order[1].tolist() == list(range(mn.shape[1]))
    for m in (0, 2):                                                                  # the neighbours are untouched
        assert np.array_equal(rn[m], good[0][m]) and np.array_equal(re[m], good[1][m])
        assert np.array_equal(order[m], good[2][m])
    with pytest.raises(ValueError, match=word):
        routes.reorder(dn, de, route=route, rank=rank)
    if "rank" not in kind:                                    # the same with a drawn ranking, from several start nodes
        for epoch in range(6):
            err = routes.reorder(dn, de, route=route, seed=1, epoch=epoch, invalid="skip")[-1]
            assert err.cpu().tolist() == [0, bit, 0]
    if kind == "disconnected":                                # the expansion's own check reports what was passed on
        bits = routes.check(_dev(rn)[0], _dev(re)[0], GDB13_ADD, GDB13_CONN).cpu().tolist()
        assert bits[1] & L.ROUTE_ERR_CONNECT and bits[0] == bits[2] == 0


def test_empty_molecules_and_an_empty_batch():
    mn = np.zeros((3, 13, 8), dtype=np.int8)
    me = np.zeros((3, 13, 13, 3), dtype=np.int8)
    mn[1, 0, 2] = 1                                                       # a single atom between two empty molecules
    for route in ("bfs", "dfs"):
        rn, re, order, err = routes.reorder(*_dev(mn, me), route=route, return_order=True, invalid="skip")
        assert err.cpu().tolist() == [L.ROUTE_ERR_EMPTY, 0, L.ROUTE_ERR_EMPTY]
        assert np.array_equal(rn.cpu().numpy(), mn) and not re.any()
        assert order[1].cpu().tolist() == [0] + [-1] * 12
        with pytest.raises(ValueError, match="no node"):
            routes.reorder(*_dev(mn, me), route=route)
        out = routes.reorder(*_dev(mn[:0], me[:0]), route=route, return_order=True)
        assert out[0].shape == (0, 13, 8) and out[1].shape == (0, 13, 13, 3) and out[2].shape == (0, 13)


# ---- RouteLoader(reorder=...) ------------------------------------------------------------------------------
def _epoch_rows(ld):
    """Per molecule of the epoch (dataset index): row 0 of its route, i.e. the molecule the loader expanded."""
    assert not ld.merge
    seen, batches = {}, []
    for (n, e, a), idx in zip(ld, ld.batch_molecules()):
        n, e, a = _host((n, e, a))
        whole = np.nonzero(a[:, -1] > 0)[0]                               # the rows whose f_term is set
        assert len(whole) == len(idx)
        for r, m in zip(whole, idx):
            seen[int(m)] = (n[r], e[r])
        batches.append(n.shape[0])
    return seen, batches


@pytest.mark.parametrize("route", ["bfs", "dfs"])
def test_route_loader_reorders_every_molecule_as_the_model_does(golden_dir, route):
    mn, me = _fixture_molecules(golden_dir)
    M = mn.shape[0]
    plain = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=5, device=DEV, merge=False)
    ld = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=5, device=DEV, merge=False,
                            reorder=route)
    per_epoch = []
    for epoch in (0, 1):
        ld.set_epoch(epoch)
        plain.set_epoch(epoch)
        seen, batches = _epoch_rows(ld)
        want_n, want_e, _ = OM.reorder(mn, me, route, seed=5, epoch=epoch, mol_ids=np.arange(M))
        assert sorted(seen) == list(range(M))
        for m in range(M):
            assert np.array_equal(seen[m][0], want_n[m]) and np.array_equal(seen[m][1], want_e[m]), (epoch, m)
        _, plain_batches = _epoch_rows(plain)
        assert len(ld) == len(plain) and batches == plain_batches         # batch count and unmerged row counts
        per_epoch.append(seen)
        # two ranks agree with the single rank, molecule for molecule
        both = {}
        for r in range(2):
            half = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=48, rank=r, world_size=2, seed=5,
                                      device=DEV, merge=False, reorder=route)
            half.set_epoch(epoch)
            both.update(_epoch_rows(half)[0])
        assert sorted(both) == list(range(M))
        assert all(np.array_equal(both[m][0], seen[m][0]) and np.array_equal(both[m][1], seen[m][1])
                   for m in range(M))
    assert any(not np.array_equal(per_epoch[0][m][1], per_epoch[1][m][1]) for m in range(M))   # epochs differ


def test_route_loader_takes_molecules_in_any_node_order_when_it_reorders(golden_dir):
    g = _golden(golden_dir, "gdb13")
    mn, me = g["mol_nodes"][:40], g["mol_edges"][:40]                     # the odd ones are not in a BFS order
    with pytest.raises(ValueError, match="lower index"):
        for _ in routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=1, device=DEV):
            pass
    ld = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=1, device=DEV, reorder="dfs")
    ld.set_epoch(3)
    for (n, e, a), idx in zip(ld, ld.batch_molecules()):
        rn, re, _ = OM.reorder(mn[idx], me[idx], "dfs", seed=1, epoch=3, mol_ids=idx)
        kn, ke, sums, _, _ = RM.merge(*RM.expand(rn, re, GDB13_ADD, GDB13_CONN), 625)
        n, e, a = _host((n, e, a))
        assert np.array_equal(n, kn) and np.array_equal(e, ke) and np.array_equal(a, sums)


def test_route_loader_without_reorder_is_the_expansion_of_the_stored_molecules(golden_dir):
    mn, me = _fixture_molecules(golden_dir)
    for merge in (True, False):
        ld = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=5, device=DEV, merge=merge,
                                reorder=None)
        ld.set_epoch(2)
        for got, idx in zip(ld, ld.batch_molecules()):
            want = routes.expand(*_dev(mn[idx], me[idx]), GDB13_ADD, GDB13_CONN, merge=merge)[:3]
            assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_reordering_loader_issues_no_synchronising_call(golden_dir):
    mn, me = _fixture_molecules(golden_dir)
    ld = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=2, device=DEV, reorder="bfs")
    for _ in ld:                                                          # warm-up: allocations, pinned staging
        pass
    acc = torch.zeros((), device=DEV)
    ld.set_epoch(1)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            for n, e, a in ld:
                acc += n.sum() + e.sum() + a.sum()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert [str(x.message) for x in w if "synchroniz" in str(x.message)] == []
    assert float(acc) > 0


@pytest.mark.parametrize("route", ["bfs", "dfs"])
def test_training_through_a_reordering_loader_learns(golden_dir, route):
    """A smoke check, not parity: every epoch sees other routes of the same 20 molecules."""
    from examples.train_fixture import constants_for
    from graphinvent_amd import dp
    from graphinvent_amd.gnn import mpnn
    from graphinvent_amd.loss import apd_kl_loss
    from graphinvent_amd.optim import FusedAdam
    mn, me = _fixture_molecules(golden_dir)
    shapes = (np.empty((1, 13, 8), np.int8), np.empty((1, 13, 13, 3), np.int8), np.empty((1, 625), np.int8))
    torch.manual_seed(7)
    model = mpnn.GGNN(constants_for(*shapes)).to(DEV).train()
    trainer = dp.DataParallel(model, FusedAdam(model.parameters(), lr=1e-3), None, loss_fn=apd_kl_loss)
    ld = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=4, device=DEV, reorder=route)
    history = []
    for epoch in range(8):
        ld.set_epoch(epoch)
        losses = [trainer.step(n, e, a) for n, e, a in ld]
        history.append(float(torch.stack(losses).mean()))
    print(f"\n{route}: mean loss per epoch {[round(x, 4) for x in history]}")
    assert np.isfinite(history).all() and history[-1] < history[0]
