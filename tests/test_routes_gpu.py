"""GPU: graphinvent_amd.routes — expand (unmerged against the reference's golden routes, merged against the numpy
model's first-occurrence merge), the input checks, RouteLoader, and a route-fed training run."""
import os
import warnings

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import routes
from tests import routes_model as RM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GDB13_ADD, GDB13_CONN = [13, 5, 3, 3], [13, 3]


def _golden(golden_dir, config):
    G = np.load(os.path.join(golden_dir, "golden_routes.npz"))
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


def _assert_unmerged(out, mn, me, ref, add, conn):
    """`out` of expand(merge=False) on molecules mn, me against ref = (rows_nodes, rows_edges, hot, row_mol, row_step)."""
    n, e, a, rm, rs = _host(out)
    width = RM.apd_width(add, conn)
    assert out[2].dtype == (torch.int8 if mn.shape[0] <= 127 else torch.float32)
    assert n.dtype == np.int8 and e.dtype == np.int8 and rm.dtype == np.int32 and rs.dtype == np.int32
    assert n.shape == ref[0].shape and e.shape == ref[1].shape and a.shape == (len(ref[2]), width)
    assert np.array_equal(n, ref[0])
    assert np.array_equal(e, ref[1])
    assert np.array_equal(a, RM.one_hot(ref[2], width, a.dtype))
    assert np.array_equal(rm, ref[3]) and np.array_equal(rs, ref[4])


@pytest.mark.parametrize("config", ["gdb13", "arom5", "chiral6"])
def test_unmerged_rows_equal_the_reference_route(golden_dir, config):
    g = _golden(golden_dir, config)
    mn, me = g["mol_nodes"], g["mol_edges"]
    ref = (g["rows_nodes"], g["rows_edges"], g["hot"], g["row_mol"], g["row_step"])
    dn, de = _dev(mn, me)
    out = routes.expand(dn, de, g["dim_f_add"], g["dim_f_conn"], merge=False)
    _assert_unmerged(out, mn, me, ref, g["dim_f_add"], g["dim_f_conn"])
    # the same with the row count from the host copies: no sizing read-back
    n_rows = int(routes.route_lengths(mn, me).sum())
    out = routes.expand(dn, de, g["dim_f_add"], g["dim_f_conn"], merge=False, n_rows=n_rows)
    _assert_unmerged(out, mn, me, ref, g["dim_f_add"], g["dim_f_conn"])
    with pytest.raises(ValueError, match="rows"):
        routes.expand(dn, de, g["dim_f_add"], g["dim_f_conn"], merge=False, n_rows=n_rows - 1)


def test_unmerged_rows_in_calls_of_1_7_and_128_molecules(golden_dir):
    """int8 APDs up to 127 molecules, fp32 above; row offsets that are not multiples of anything."""
    g = _golden(golden_dir, "gdb13")
    mn, me = g["mol_nodes"], g["mol_edges"]
    assert mn.shape[0] >= 136
    lo = 0
    for size in (1, 7, 128, mn.shape[0] - 136):
        if size == 0:
            continue
        hi = lo + size
        rows = (g["row_mol"] >= lo) & (g["row_mol"] < hi)
        ref = (g["rows_nodes"][rows], g["rows_edges"][rows], g["hot"][rows], g["row_mol"][rows] - lo,
               g["row_step"][rows])
        out = routes.expand(*_dev(mn[lo:hi], me[lo:hi]), g["dim_f_add"], g["dim_f_conn"], merge=False)
        _assert_unmerged(out, mn[lo:hi], me[lo:hi], ref, g["dim_f_add"], g["dim_f_conn"])
        lo = hi


def _assert_merged(out, mn, me, add, conn):
    width = RM.apd_width(add, conn)
    kn, ke, sums, km, ks = RM.merge(*RM.expand(mn, me, add, conn), width)
    n, e, a, rm, rs = _host(out)
    assert out[2].dtype == (torch.int8 if mn.shape[0] <= 127 else torch.float32)
    assert n.shape == kn.shape and np.array_equal(n, kn) and np.array_equal(e, ke)
    assert np.array_equal(a.astype(np.int64), sums) and np.array_equal(a, sums.astype(a.dtype))
    assert np.array_equal(rm, km) and np.array_equal(rs, ks)
    return sums


@pytest.mark.parametrize("config", ["gdb13", "arom5", "chiral6"])
def test_merged_rows_equal_the_first_occurrence_merge(golden_dir, config):
    g = _golden(golden_dir, config)
    mn, me = g["mol_nodes"], g["mol_edges"]
    dn, de = _dev(mn, me)
    out = routes.expand(dn, de, g["dim_f_add"], g["dim_f_conn"])
    sums = _assert_merged(out, mn, me, g["dim_f_add"], g["dim_f_conn"])
    assert out[0].shape[0] < len(g["hot"]) and sums.max() > 1            # something did merge
    again = routes.expand(dn, de, g["dim_f_add"], g["dim_f_conn"])       # two runs: identical bytes
    assert all(torch.equal(x, y) for x, y in zip(out, again))
    small = routes.expand(*_dev(mn[:20], me[:20]), g["dim_f_add"], g["dim_f_conn"])   # <= 127 molecules: int8 sums
    _assert_merged(small, mn[:20], me[:20], g["dim_f_add"], g["dim_f_conn"])


def test_merge_of_300_copies_sums_past_127_in_fp32(golden_dir):
    g = _golden(golden_dir, "gdb13")
    pick = np.resize(np.array([0, 23, 5]), 300)                           # few distinct molecules, interleaved
    mn, me = g["mol_nodes"][pick], g["mol_edges"][pick]
    out = routes.expand(*_dev(mn, me), g["dim_f_add"], g["dim_f_conn"])
    sums = _assert_merged(out, mn, me, g["dim_f_add"], g["dim_f_conn"])
    assert out[2].dtype == torch.float32 and sums.max() > 127             # entries past what int8 holds
    assert (sums[:, -1] == 100).sum() == 3                               # each whole molecule, 100 times


@pytest.mark.parametrize("mask", [0, 0x3, 0xFFFF0000])
def test_colliding_hashes_are_told_apart_by_the_byte_compare(golden_dir, mask):
    """With the hash cut to a few bits (mask 0: one bucket for all) different graphs share table buckets; the
    result must not change."""
    g = _golden(golden_dir, "gdb13")
    pick = np.concatenate([np.arange(12), np.arange(6), np.arange(20, 30)])
    mn, me = g["mol_nodes"][pick], g["mol_edges"][pick]
    dn, de = _dev(mn, me)
    out = routes.expand(dn, de, g["dim_f_add"], g["dim_f_conn"], _hash_mask=mask)
    _assert_merged(out, mn, me, g["dim_f_add"], g["dim_f_conn"])
    full = routes.expand(dn, de, g["dim_f_add"], g["dim_f_conn"])
    assert all(torch.equal(x, y) for x, y in zip(out, full))


def _break(kind, nodes, edges):
    """Make molecule 1 of the batch invalid in one way; returns the expected error bit."""
    n = int(nodes[1].any(axis=1).sum())
    last = n - 1
    if kind == "no_lower_neighbour":
        edges[1, last] = 0
        edges[1, :, last] = 0
        return L.ROUTE_ERR_CONNECT
    if kind == "asymmetric":
        j, t = np.argwhere(edges[1, last])[0]
        edges[1, j, last, t] = 0
        return L.ROUTE_ERR_ASYMMETRIC
    if kind == "two_bond_types":
        j, t = np.argwhere(edges[1, last])[0]
        edges[1, last, j, (t + 1) % 3] = edges[1, j, last, (t + 1) % 3] = 1
        return L.ROUTE_ERR_MULTI_BOND
    if kind == "not_one_hot":
        nodes[1, 0, :5] = 0
        nodes[1, 0, [0, 1]] = 1
        return L.ROUTE_ERR_ONEHOT
    if kind == "not_0_1":
        j, t = np.argwhere(edges[1, last])[0]
        edges[1, last, j, t] = edges[1, j, last, t] = 2
        return L.ROUTE_ERR_VALUE
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["no_lower_neighbour", "asymmetric", "two_bond_types", "not_one_hot", "not_0_1"])
@pytest.mark.parametrize("merge", [False, True])
def test_invalid_molecules_set_their_bit_and_leave_their_neighbours_alone(golden_dir, kind, merge):
    g = _golden(golden_dir, "gdb13")
    mn, me = g["mol_nodes"][:3].copy(), g["mol_edges"][:3].copy()          # three fixture molecules
    bit = _break(kind, mn, me)
    dn, de = _dev(mn, me)
    bits = routes.check(dn, de, GDB13_ADD, GDB13_CONN).cpu().tolist()
    assert bits[0] == 0 and bits[2] == 0 and bits[1] & bit, (kind, bits)
    with pytest.raises(ValueError) as err:
        routes.expand(dn, de, GDB13_ADD, GDB13_CONN, merge=merge)
    assert routes.ERROR_MESSAGES[bit] in str(err.value)
    with pytest.raises(ValueError):
        routes.expand(dn, de, GDB13_ADD, GDB13_CONN, merge=merge,
                      n_rows=int(routes.route_lengths(mn, me).sum()))
    out = routes.expand(dn, de, GDB13_ADD, GDB13_CONN, merge=merge, invalid="skip")
    vn, ve = mn[[0, 2]], me[[0, 2]]
    if merge:
        kn, ke, sums, km, ks = RM.merge(*RM.expand(vn, ve, GDB13_ADD, GDB13_CONN), 625)
    else:
        kn, ke, hot, km, ks = RM.expand(vn, ve, GDB13_ADD, GDB13_CONN)
        sums = RM.one_hot(hot, 625)
    n, e, a, rm, rs = _host(out)
    assert np.array_equal(n, kn) and np.array_equal(e, ke) and np.array_equal(a.astype(np.int64), sums)
    assert np.array_equal(rm, np.array([0, 2])[km]) and np.array_equal(rs, ks)


def test_empty_and_padding_violations():
    mn = np.zeros((2, 13, 8), dtype=np.int8)
    me = np.zeros((2, 13, 13, 3), dtype=np.int8)
    mn[1, 1, [0, 5]] = 1                                                  # node 1 present, node 0 not
    bits = routes.check(*_dev(mn, me), GDB13_ADD, GDB13_CONN).cpu().tolist()
    assert bits[0] & L.ROUTE_ERR_EMPTY and bits[1] & L.ROUTE_ERR_PADDING


# ---- RouteLoader ------------------------------------------------------------------------------------------
def _row_keys(n, e, a):
    return sorted(n[r].tobytes() + e[r].tobytes() + a[r].astype(np.int64).tobytes() for r in range(n.shape[0]))


def test_route_loader_epoch_equals_the_per_batch_merged_expansion(golden_dir):
    mn, me = _fixture_molecules(golden_dir)
    assert mn.shape[0] == 20
    for merge in (True, False):
        ld = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=5, device=DEV, merge=merge)
        for epoch in (0, 1):
            ld.set_epoch(epoch)
            groups = ld.batch_molecules()
            assert len(groups) == len(ld) and sorted(np.concatenate(groups).tolist()) == list(range(20))
            got = [_host(b) for b in ld]
            assert len(got) == len(groups)
            for (n, e, a), idx in zip(got, groups):
                rows = RM.expand(mn[idx], me[idx], GDB13_ADD, GDB13_CONN)
                assert rows[0].shape[0] <= 64
                if merge:
                    kn, ke, sums, _, _ = RM.merge(*rows, 625)
                else:
                    kn, ke, sums = rows[0], rows[1], RM.one_hot(rows[2], 625)
                assert a.dtype == np.int8
                assert _row_keys(n, e, a) == _row_keys(kn, ke, sums)
                assert np.array_equal(n, kn) and np.array_equal(e, ke) and np.array_equal(a, sums)


def test_two_ranks_partition_the_molecules(golden_dir):
    mn, me = _fixture_molecules(golden_dir)
    lds = [routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=48, rank=r, world_size=2, seed=1, device=DEV)
           for r in range(2)]
    mols = [np.concatenate(ld.batch_molecules()) for ld in lds]
    assert len(lds[0]) == len(lds[1])
    assert sorted(np.concatenate(mols).tolist()) == list(range(20)) and len(mols[0]) == len(mols[1]) == 10
    for ld, mine in zip(lds, mols):
        wholes = 0
        for n, e, a in ld:
            wholes += int((a[:, -1] > 0).sum())                           # one terminate row per molecule
        assert wholes == len(mine)


def _sync_debug_honoured() -> bool:
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            torch.ones(1, device=DEV).item()
        return any("synchroniz" in str(x.message) for x in w)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_route_loader_iteration_issues_no_synchronising_call(golden_dir):
    """The method of profiles/eval/README.md: torch.cuda.set_sync_debug_mode("warn") around the iteration.  The
    loader's host side waits for events of its own side stream only; the consumer's stream is never waited on."""
    mn, me = _fixture_molecules(golden_dir)
    ld = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=2, device=DEV)
    for _ in ld:                                                          # warm-up: allocations, pinned staging
        pass
    print(f"\nset_sync_debug_mode honoured on this build: {_sync_debug_honoured()}")
    acc = torch.zeros((), device=DEV)
    ld.set_epoch(1)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            for n, e, a in ld:
                acc += n.sum() + e.sum() + a.sum()                         # the consumer's work, on its own stream
    finally:
        torch.cuda.set_sync_debug_mode(0)
    syncs = [str(x.message) for x in w if "synchroniz" in str(x.message)]
    assert syncs == []
    assert float(acc) > 0


# ---- end to end -------------------------------------------------------------------------------------------
def _train(golden_dir, feed, steps=30):
    """`steps` Adam steps of a GGNN at the fixture's shape from a fixed seed; the per-step losses (host floats)."""
    from examples.train_fixture import constants_for
    from graphinvent_amd import dp
    from graphinvent_amd.gnn import mpnn
    from graphinvent_amd.loss import apd_kl_loss
    from graphinvent_amd.optim import FusedAdam
    shapes = (np.empty((1, 13, 8), np.int8), np.empty((1, 13, 13, 3), np.int8), np.empty((1, 625), np.int8))
    torch.manual_seed(7)
    model = mpnn.GGNN(constants_for(*shapes)).to(DEV).train()
    trainer = dp.DataParallel(model, FusedAdam(model.parameters(), lr=1e-3), None, loss_fn=apd_kl_loss)
    losses, k = [], 0
    while k < steps:
        for n, e, a in feed():
            losses.append(trainer.step(n, e, a))
            k += 1
            if k == steps:
                break
    return torch.stack(losses).cpu().numpy()


def test_route_fed_training_equals_tensor_fed_training(golden_dir):
    """30 Adam steps fed by RouteLoader against the same steps fed the numpy model's rows as plain tensors.  The
    inputs are bit-identical, so the only admissible difference is the step's own run-to-run variation, measured
    here by running the tensor-fed steps twice from identical seeds."""
    mn, me = _fixture_molecules(golden_dir)
    ld = routes.RouteLoader(mn, me, GDB13_ADD, GDB13_CONN, batch_size=64, seed=4, device=DEV)
    epochs = []
    for epoch in range(30):                                               # at most 30 epochs are needed for 30 steps
        batches = []
        for idx in routes.plan_batches(ld.lengths, 64, seed=4, epoch=epoch):
            kn, ke, sums, _, _ = RM.merge(*RM.expand(mn[idx], me[idx], GDB13_ADD, GDB13_CONN), 625)
            batches.append(_dev(kn, ke, sums.astype(np.int8)))
        epochs.append(batches)

    def tensor_feed():
        state = {"epoch": 0}

        def feed():
            out = epochs[state["epoch"]]
            state["epoch"] += 1
            return out
        return feed

    def route_feed():
        state = {"epoch": 0}

        def feed():
            ld.set_epoch(state["epoch"])
            state["epoch"] += 1
            return ld
        return feed

    t1 = _train(golden_dir, tensor_feed())
    t2 = _train(golden_dir, tensor_feed())
    r = _train(golden_dir, route_feed())
    assert np.isfinite(t1).all() and t1[-1] < t1[0]
    spread = np.abs(t1 - t2)
    diff = np.abs(r - t1)
    print(f"\ntensor-fed run-to-run max |d loss| {spread.max():.3e}; route-fed vs tensor-fed max {diff.max():.3e}")
    if spread.max() == 0:
        assert np.array_equal(r, t1)
    else:
        assert diff.max() <= spread.max()
