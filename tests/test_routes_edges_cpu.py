"""CPU: the seam cases of tests/route_cases.py.  Every case satisfies the condition it was built for (asserted here,
so tests/test_routes_edges_gpu.py can rely on it), the numpy model's rows pass the replay, and routes.route_lengths
equals the model's lengths.  No device compute is issued."""
import functools

import numpy as np
import pytest

from graphinvent_amd import routes
from tests import reorder_model as OM
from tests import route_cases as RC
from tests import routes_model as RM


@functools.lru_cache(maxsize=None)
def _summary(name):
    """The model's expansion of a case, once per module; the rows themselves are not kept."""
    c = RC.case(name)
    rows = RM.expand(c.nodes, c.edges, c.add, c.conn)
    out = {"case": c, "rows": len(rows[2]), "lengths": np.bincount(rows[3], minlength=c.M), "steps": None,
           "replay_error": None}
    try:
        out["steps"] = RC.replay_batch(rows[0], rows[1], rows[2], rows[3], c.nodes, c.edges, c.add, c.conn)
    except AssertionError as err:
        out["replay_error"] = str(err) or "assertion failed"
    if "merged" in c.modes:
        kn, _, sums, km, _ = RM.merge(*rows, c.width)
        out["kept"], out["max_sum"], out["kept_mol"] = len(kn), int(sums.max()), km
    return out


@pytest.mark.parametrize("name", RC.NAMES)
def test_cases_are_well_formed_and_inside_the_limits(name):
    c = RC.case(name)
    RC.well_formed(c.nodes, c.edges, c.seg)
    assert c.N <= 128 and c.Fe <= 8 and 1 <= len(c.seg) <= 4
    d = routes._route_dims(c.M, c.N, c.Fn, c.Fe, c.add, c.conn)
    assert d.apd_width == c.width == RM.apd_width(c.add, c.conn)


@pytest.mark.parametrize("name", RC.NAMES)
def test_model_rows_pass_the_replay(name):
    s = _summary(name)
    assert s["replay_error"] is None
    assert [len(x) for x in s["steps"]] == (s["lengths"] - 2).tolist()      # one decoded bond per bond


@pytest.mark.parametrize("name", RC.NAMES)
def test_route_lengths_equal_the_models(name):
    s = _summary(name)
    lengths = routes.route_lengths(s["case"].nodes, s["case"].edges)
    assert lengths.dtype == np.int64 and np.array_equal(lengths, s["lengths"])
    assert int(lengths.sum()) == s["rows"]


def _lower(edges, i):
    return set(np.nonzero(edges[i, :i].any(axis=1))[0].tolist())


@pytest.mark.parametrize("N", RC.SEAM_N)
def test_node_seam_batches(N):
    c = RC.case(f"nodes-{N}")
    n_nodes = c.nodes.any(axis=2).sum(axis=1).tolist()
    assert n_nodes[:3] == [N, max(N - 1, 1), 1] and c.M == (4 if N >= 65 else 3)
    assert np.array_equal(c.edges[1], RC.truncated(c.nodes[0], c.edges[0], max(N - 1, 1))[1])
    n_bonds = int(c.edges[0].any(axis=2).sum()) // 2
    assert n_bonds >= (N - 1) + (N // 4) * 3 // 4                         # the tree and most of its ring closures
    if N >= 63:
        assert {int(t) for t in np.nonzero(c.edges[0])[2]} == {0, 1, 2}
    if N < 65:
        return
    e = c.edges[3]
    assert n_nodes[3] == N
    assert len(_lower(e, 64)) >= 2                                        # node 64: two trips of the lower-node loops
    if N - 1 > 64:                                                        # at N = 65 node 64 IS the last node
        low = _lower(e, N - 1)
        assert any(j < 64 for j in low) and any(j >= 64 for j in low)
        assert any(j + 64 in low for j in low)                            # one lane, both trips


def test_complete_graph_reaches_step_8129():
    s = _summary("k128")
    assert s["rows"] == 8130 == 2 + 128 * 127 // 2
    steps = s["steps"][0]
    assert len(steps) == 8128 and max(k for k, _, _, _ in steps) == 8128
    # the route's last step, 8129, removes node 0; the last bond step sets bits 6 .. 12 of the 13-bit field
    assert s["lengths"][0] - 1 == 8129 and 8128 & 0x1FC0 == 0x1FC0
    assert s["case"].edges.nbytes * 8130 > 130e6


def test_every_type_has_a_step_above_4095():
    s = _summary("steps-fe4")
    c = s["case"]
    n_bonds = int(c.edges[0].any(axis=2).sum()) // 2
    assert n_bonds >= 4200 and (c.N, c.Fe) == (128, 4)
    i, j, t = np.nonzero(c.edges[0])
    assert np.array_equal(t, (i + j) % 4)
    top = {}
    for k, _, _, t in s["steps"][0]:
        top[t] = max(top.get(t, 0), k)
    assert sorted(top) == [0, 1, 2, 3] and min(top.values()) > 4095       # bit 12 of the step under every type


def test_node_127_has_type_0_codes_that_look_like_type_markers():
    s = _summary("codes-fe8")
    c = s["case"]
    assert (c.N, c.Fe) == (128, 8) and 590 <= s["rows"] - 2 <= 610
    assert {int(t) for t in np.nonzero(c.edges[0])[2]} == set(range(8))
    mine = [(k, j, t) for k, i, j, t in s["steps"][0] if i == 127]
    by_type = {t: sorted(k for k, _, tt in mine if tt == t) for t in range(8)}
    assert len(by_type[0]) >= 9 and all(len(by_type[t]) >= 1 for t in range(1, 8))
    assert sorted(k for k, _, _ in mine) == list(range(1, len(mine) + 1))  # node 127's first step is 1
    # descending (type, index): the other types come first, so type 0 holds the node's last steps, and its first
    # one is a number that is also a `type + 1` marker ...
    assert by_type[0] == list(range(len(mine) - len(by_type[0]) + 1, len(mine) + 1))
    # (and an ascending sweep would hand type 0 the codes 1 .. 9, eight of them markers of types the node has)
    assert by_type[0][0] <= c.Fe
    low = {j for _, j, _ in mine}
    assert any(j < 64 for j in low) and any(j >= 64 for j in low)


@pytest.mark.parametrize("shape", range(len(RC.PIECE_SHAPES)))
def test_piece_batches_end_inside_a_16_byte_piece(shape):
    N, seg, Fe = RC.PIECE_SHAPES[shape]
    good = []
    for M in RC.PIECE_M:
        s = _summary(f"piece-{shape}-{M}")
        c = s["case"]
        assert (c.M, c.N, c.seg, c.Fe) == (M, N, seg, Fe)
        totals = [s["rows"] * N * c.Fn, s["rows"] * N * N * Fe, s["rows"] * c.width * c.apd_itemsize]
        good.append(all(x % 16 for x in totals))
        assert "kept" in s and s["kept"] <= s["rows"]
    assert (N * sum(seg)) % 16 and (N * N * Fe) % 16 and c.width % 16      # no pitch is a whole number of pieces
    assert any(good)


@pytest.mark.parametrize("M", RC.SCAN_M)
def test_scan_batches_merge_to_a_handful_of_rows(M):
    s = _summary(f"scan-{M}")
    c = s["case"]
    assert c.M == M and c.N == 3
    assert len({c.nodes[m].tobytes() + c.edges[m].tobytes() for m in range(M)}) == 6
    assert s["rows"] > 2 * M and s["kept"] <= 6 * 5 and s["max_sum"] > 127
    assert s["kept_mol"].max() < 64                                       # everything kept sits in the first rows


def test_distinct_batch_keeps_more_rows_than_a_scan_chunk():
    s = _summary("scan-distinct")
    c = s["case"]
    assert len({c.nodes[m].tobytes() + c.edges[m].tobytes() for m in range(c.M)}) == c.M
    assert 1024 < s["kept"] < s["rows"]


def test_segment_and_sum_cases():
    assert [len(RC.case(n).seg) for n in ("seg-1", "seg-4")] == [1, 4]
    for name in ("seg-1", "seg-4"):
        c = RC.case(name)
        assert (c.M, c.N, c.Fe) == (40, 9, 3)
    a, b = _summary("sum-127"), _summary("sum-128")
    assert (a["case"].M, a["max_sum"], a["case"].apd_itemsize) == (127, 127, 1)
    assert (b["case"].M, b["max_sum"], b["case"].apd_itemsize) == (128, 128, 4)
    assert a["kept"] == b["kept"] == a["lengths"][0]


@pytest.mark.parametrize("route", RC.REORDER_ROUTES)
@pytest.mark.parametrize("N", RC.REORDER_N)
def test_reordered_molecules_are_valid_input_and_replay(N, route):
    nodes, edges, rank = RC.reorder_inputs(N, route)
    assert nodes.shape[0] == 3 and nodes.any(axis=2).sum(axis=1).tolist() == [N, N - 1, N // 2 + 1]
    with pytest.raises(AssertionError):
        RC.well_formed(nodes, edges, RC.REORDER_SEG)                      # the input order is NOT a valid one
    rn_, re_, order = OM.reorder(nodes, edges, route, rank=rank)
    assert any(order[m, 0] != 0 for m in range(3))
    RC.well_formed(rn_, re_, RC.REORDER_SEG)
    add, conn = [N] + RC.REORDER_SEG + [RC.REORDER_FE], [N, RC.REORDER_FE]
    rows = RM.expand(rn_, re_, add, conn)
    RC.replay_batch(rows[0], rows[1], rows[2], rows[3], rn_, re_, add, conn)
    assert np.array_equal(routes.route_lengths(nodes, edges), np.bincount(rows[3]))
