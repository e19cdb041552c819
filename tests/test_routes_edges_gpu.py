"""GPU: routes.expand at the seams of csrc/gi_route.hip (tests/route_cases.py; tests/test_routes_edges_cpu.py asserts
what each case reaches) against the step-by-step numpy model, byte for byte: nodes, edges, APDs and their dtype,
row_mol, row_step, unmerged and merged.  The device's unmerged rows also go through the replay, which shares nothing
with the model, and routes.check must find every molecule valid.

The model of a case is computed once and shared by the case's modes (they are adjacent in the parametrisation);
large outputs come to the host in slices of whole molecules."""
import functools

import numpy as np
import pytest
import torch

from graphinvent_amd import routes
from tests import reorder_model as OM
from tests import route_cases as RC
from tests import routes_model as RM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLICE_BYTES = 64 << 20


@functools.lru_cache(maxsize=1)
def _model(name):
    """(case, unmerged model rows, memo of the merged model rows) of the latest case only: steps-fe4's are 288 MB."""
    c = RC.case(name)
    return c, RM.expand(c.nodes, c.edges, c.add, c.conn), {}


def _merged_model(name):
    c, ref, memo = _model(name)
    if "merged" not in memo:
        memo["merged"] = RM.merge(*ref, c.width)
    return memo["merged"]


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _same(got, want):
    """Equal dtype, shape and bytes (not merely equal values)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(np.ascontiguousarray(got).reshape(-1).view(np.uint8),
                          np.ascontiguousarray(want).reshape(-1).view(np.uint8))


def _apd_dtype(M):
    return (torch.int8, np.int8) if M <= 127 else (torch.float32, np.float32)


def _slices(starts, row_bytes):
    """[a, b) row ranges cut at entries of `starts` (ascending row offsets, the total last), about SLICE_BYTES each."""
    out, a = [], 0
    for b in starts[1:]:
        if (b - a) * row_bytes >= SLICE_BYTES or b == starts[-1]:
            if b > a:
                out.append((int(a), int(b)))
            a = b
    return out


def _check_unmerged(out, c, ref, replay=True):
    n, e, a, rm, rs = out
    R = len(ref[2])
    tdt, ndt = _apd_dtype(c.M)
    assert n.dtype == torch.int8 and e.dtype == torch.int8 and a.dtype == tdt
    assert tuple(n.shape) == (R, c.N, c.Fn) and tuple(e.shape) == (R, c.N, c.N, c.Fe) and tuple(a.shape) == (R, c.width)
    h_rm, h_rs = rm.cpu().numpy(), rs.cpu().numpy()
    _same(h_rm, ref[3])
    _same(h_rs, ref[4])
    assert (np.diff(h_rm) >= 0).all()
    starts = np.searchsorted(ref[3], np.arange(c.M + 1))                  # whole molecules per slice: the replay's unit
    for lo, hi in _slices(starts, c.N * c.N * c.Fe + c.N * c.Fn + c.width * a.element_size()):
        hn, he, ha = n[lo:hi].cpu().numpy(), e[lo:hi].cpu().numpy(), a[lo:hi].cpu().numpy()
        _same(hn, ref[0][lo:hi])
        _same(he, ref[1][lo:hi])
        _same(ha, RM.one_hot(ref[2][lo:hi], c.width, ndt))
        if replay:
            assert (ha.sum(axis=1) == 1).all()
            m0, m1 = int(h_rm[lo]), int(h_rm[hi - 1]) + 1
            RC.replay_batch(hn, he, ha.argmax(axis=1), h_rm[lo:hi] - m0, c.nodes[m0:m1], c.edges[m0:m1], c.add, c.conn)


def _check_merged(out, c, want):
    n, e, a, rm, rs = out
    kn, ke, sums, km, ks = want
    tdt, ndt = _apd_dtype(c.M)
    assert n.dtype == torch.int8 and e.dtype == torch.int8 and a.dtype == tdt
    assert sums.max() <= (127 if c.M <= 127 else 2 ** 24)
    _same(rm.cpu().numpy(), km)
    _same(rs.cpu().numpy(), ks)
    K = len(km)
    assert n.shape[0] == e.shape[0] == a.shape[0] == K
    step = max(1, SLICE_BYTES // (c.N * c.N * c.Fe + c.N * c.Fn + c.width * a.element_size()))
    for lo in range(0, K, step):
        hi = min(K, lo + step)
        _same(n[lo:hi].cpu().numpy(), kn[lo:hi])
        _same(e[lo:hi].cpu().numpy(), ke[lo:hi])
        _same(a[lo:hi].cpu().numpy(), sums[lo:hi].astype(ndt))


@pytest.mark.parametrize("name, mode", [(name, mode) for name in RC.NAMES for mode in RC.modes(name)])
def test_expand_equals_the_model_byte_for_byte(name, mode):
    """Measured on an MI355X host, model, transfers and replay included: all 71 cases of this module 4.3 s; the slowest
    are k128 (8130 rows, 133 MB of edges) at 0.29 s unmerged and 0.26 s merged, and steps-fe4 (4392 rows, 288 MB)
    at 0.27 s.  None needed shrinking."""
    c, ref, _ = _model(name)
    dn, de = _dev(c.nodes, c.edges)
    if mode == "unmerged":
        bits = routes.check(dn, de, c.add, c.conn)
        assert bits.dtype == torch.int32 and bits.cpu().tolist() == [0] * c.M
        _check_unmerged(routes.expand(dn, de, c.add, c.conn, merge=False), c, ref)
    elif mode == "merged":
        out = routes.expand(dn, de, c.add, c.conn)
        want = _merged_model(name)
        _check_merged(out, c, want)
        if name.startswith("scan-"):
            assert out[0].shape[0] == len(want[0]) and int(routes.route_lengths(c.nodes, c.edges).sum()) == len(ref[2])
            assert (np.diff(out[3].cpu().numpy()) >= 0).all()
        if name.startswith("sum-"):
            assert int(out[2].max()) == c.M and out[2].dtype == _apd_dtype(c.M)[0]
    else:                                                                 # the row count from the host copies
        n_rows = int(routes.route_lengths(c.nodes, c.edges).sum())
        assert n_rows == len(ref[2])
        _check_unmerged(routes.expand(dn, de, c.add, c.conn, merge=False, n_rows=n_rows), c, ref, replay=False)
        _check_merged(routes.expand(dn, de, c.add, c.conn, n_rows=n_rows), c, _merged_model(name))


@pytest.mark.parametrize("route", RC.REORDER_ROUTES)
@pytest.mark.parametrize("N", RC.REORDER_N)
def test_reorder_then_expand_equals_the_two_models(N, route):
    nodes, edges, rank = RC.reorder_inputs(N, route)
    want_n, want_e, want_order = OM.reorder(nodes, edges, route, rank=rank)
    got_n, got_e, got_order = routes.reorder(*_dev(nodes, edges), route=route, rank=rank, return_order=True)
    _same(got_order.cpu().numpy(), want_order)
    _same(got_n.cpu().numpy(), want_n)
    _same(got_e.cpu().numpy(), want_e)
    add, conn = [N] + RC.REORDER_SEG + [RC.REORDER_FE], [N, RC.REORDER_FE]
    c = RC.Case(f"reorder-{N}-{route}", want_n, want_e, RC.REORDER_SEG)
    assert routes.check(got_n, got_e, add, conn).cpu().tolist() == [0, 0, 0]
    _check_unmerged(routes.expand(got_n, got_e, add, conn, merge=False), c, RM.expand(want_n, want_e, add, conn))
