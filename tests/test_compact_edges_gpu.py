"""-m gpu: graph_compact (graphinvent_amd/csrc/gi_compact.hip) bit-exactly against the numpy model
tests/ref_dataflow.py::compact at the limits of its axes: the NMAX = 32 / 64 / 128 fill instantiations and the 64-bit
word seam of its bit masks, 1 and 8 bond types (mask 0xFF in a signed char), 1023 / 1024 / 1025 slots and edges (the
chunked scans), 255 / 256 / 257 feature classes, 2048 pass-0 rows, feature rows of 32 / 33 / 62 / 63 / 64 bits, int8
inputs everywhere, and the bounded (host-sync-free) mode at exactly tight bounds and one short of them.  Integer work
and small exact counts: every comparison is np.array_equal.  The inputs are those tests/test_compact_edges_cpu.py
checks the model on."""
import numpy as np
import pytest
import torch

from graphinvent_amd import ops, synthetic
from tests import compact_cases as K
from tests import ref_dataflow as D
from tests.compact_cases import _compact_case, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = ("f32", "i8")
NODEDUP = pytest.mark.parametrize("nodedup", [False, True], ids=["shared", "nodedup"])


def _both_dtypes(n8, e8, H=16, nodedup=False):
    """fp32 and int8 inputs, each bit-exact against the model; both must produce the same node rows."""
    g, hx, ref = _compact_case(n8, e8, H=H, nodedup=nodedup, in_dtype="f32")
    g8, hx8, _ = _compact_case(n8, e8, H=H, nodedup=nodedup, in_dtype="i8")
    assert torch.equal(hx, hx8)
    return g, ref


# ---- node count: fill instantiations (N <= 32, <= 64, <= 128) and bit 63 / 64 of a row and a column -------------
@NODEDUP
@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 63, 64, 65, 66, 127, 128])
def test_compact_node_count_seam(N, nodedup):
    g, ref = _both_dtypes(*K.seam_graphs(N, 3), nodedup=nodedup)
    assert (g.E > 0) == (N > 1)


# ---- bond types: Fe = 1 .. 8, the sign bit of the cell mask, the f < Fe guards ----------------------------------
@NODEDUP
@pytest.mark.parametrize("Fe", [1, 2, 5, 7, 8])
def test_compact_bond_type_axis(Fe, nodedup):
    g, ref = _both_dtypes(*K.seam_graphs(65, Fe), nodedup=nodedup)
    assert list(g.Ut)[Fe - 1] > 0


@NODEDUP
@pytest.mark.parametrize("N,Fe", [(5, 8), (33, 8), (128, 8), (128, 1)])
def test_compact_every_bond_type_on_every_pair(N, Fe, nodedup):
    g, ref = _both_dtypes(*K.all_types_graph(N, Fe), nodedup=nodedup)
    assert g.E == N * (N - 1) * Fe + 2 and g.U == (g.E if nodedup else N * Fe + 2)


# ---- slot count: the running total of compact_scan_kernel across 1024-element chunks -------------------------------
@pytest.mark.parametrize("B,N", [(341, 3), (256, 4), (205, 5), (683, 3)], ids=["1023", "1024", "1025", "2049"])
def test_compact_slot_count_seam(B, N):
    g, ref = _both_dtypes(*K.slot_count_batch(B, N))
    assert g.cidx[-1].item() == g.S - 1 and g.D0 > 0


# ---- class_csr_kernel: E below, at and above its 1024 thread chunks, one pass-0 row and several ------------------
@pytest.mark.parametrize("classes", [1, 3], ids=["D0=1", "D0=9"])
@pytest.mark.parametrize("E", [1, 2, 1023, 1024, 1025, 2049])
def test_compact_class_csr_seam(E, classes):
    g, ref = _both_dtypes(*K.edge_count_batch(E, classes))
    assert g.E == E and g.class_csr
    assert g.D0 == (1 if classes == 1 else (9 if E >= 1023 else ref["D0"]))
    assert g.cls_off[g.D0].item() == E


# ---- class limit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,D0", [(1, 1), (255, 255), (256, 256), (257, 0)])
def test_compact_class_limit(Q, D0):
    g, ref = _both_dtypes(*K.class_batch(Q, 3))
    assert g.D0 == D0 and (g.cmat is None) == (D0 == 0)


@pytest.mark.parametrize("Fe,D0", [(8, 2048), (5, 1280)], ids=["two_scan_chunks", "type_boundary_inside_a_chunk"])
def test_compact_every_class_under_every_bond_type(Fe, D0):
    g, ref = _both_dtypes(*K.class_batch(256, Fe, all_types=True))
    assert g.D0 == D0 and g.E == g.U == 512 * Fe


# ---- feature width: key_hi from Fn = 33, shortcut off from Fn = 63 ------------------------------------------------
@pytest.mark.parametrize("Fn,D0", [(32, 4), (33, 4), (62, 4), (63, 0), (64, 0)])
def test_compact_feature_width(Fn, D0):
    g, ref = _both_dtypes(*K.wide_feature_batch(Fn), H=64)
    assert g.D0 == D0
    if D0:          # the class order is the order of the unsigned 64-bit patterns
        pat = [sum(1 << b for b in bits) for bits in K.wide_feature_bits(Fn)]
        key = [(0, pat[0]), (0, pat[1]), (1, pat[1]), (1, pat[2])]          # (bond type, pattern) of the senders
        slot = [0, 1, 1, 2]
        order = sorted(range(4), key=lambda i: key[i])
        assert g.d_src.cpu().tolist() == [slot[i] for i in order]


# ---- node values outside the 0/1 contract, int8 ----------------------------------------------------------------
@pytest.mark.parametrize("value", [2, -1])
def test_compact_int8_node_value_switches_the_shortcut_off(value):
    n8, e8 = K.seam_graphs(33, 3)
    n8[1, 5, 2] = value
    g, hx0, ref = _compact_case(n8, e8, in_dtype="i8")
    assert g.D0 == 0 and g.cmat is None and g.E > 0
    row = int(ref["cidx"][33 + 5])
    assert hx0[row, 2].item() == float(value) and hx0[row, 16 + 2].item() == float(value)
    _compact_case(n8, e8, in_dtype="f32")


@pytest.mark.parametrize("value", [2, -1])
def test_compact_int8_edge_value_is_refused(value):
    n8, e8 = K.seam_graphs(33, 3)
    e8[2, 1, 0, 1] = value
    with pytest.raises(ValueError, match="0 or 1"):
        ops.compact(to_dev(n8, "i8"), to_dev(e8, "i8"), 16)


# ------------------------------------------------------------------------------------------------
# bounded (host-sync-free) mode: ops.compact_bounded called directly
# ------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC0BEEF           # (as fp32: a NaN no kernel produces)
CNT_S, CNT_E, CNT_ERR, CNT_U, CNT_UT, CNT_ET, CNT_D0 = 0, 1, 2, 3, 4, 12, 20
MAX_GROUPS = 8


class Workspace:
    """The `lay_ws` callback: hands out a view into a larger buffer filled with SENTINEL."""
    FRONT, SPARE_ROWS = 64, 8

    def __init__(self, Fn, H=16):
        self.Fn, self.H, self.ldhx = Fn, H, ops.r4(H + Fn)

    def __call__(self, S_b, E_b, U_b, D0_b):
        self.n_rows = S_b + 1 + self.SPARE_ROWS
        self.buf = torch.full((self.FRONT + self.n_rows * self.ldhx,), SENTINEL, dtype=torch.int32, device=DEV)
        return self.buf.view(torch.float32)[self.FRONT:], self.ldhx, self.H

    def front(self):
        return self.buf[:self.FRONT].cpu().numpy()

    def rows(self, dtype=np.int32):
        return self.buf[self.FRONT:].cpu().numpy().view(dtype).reshape(self.n_rows, self.ldhx)


def _bounded(n8, e8, in_dtype, e_bound, d0_bound, sticky=None):
    ws = Workspace(n8.shape[2])
    g, _ = ops.compact_bounded(to_dev(n8, in_dtype), to_dev(e8, in_dtype), ws, e_bound, d0_bound, class_csr=True,
                               sticky_err=sticky)
    torch.cuda.synchronize()
    gfix = g.gfix.cpu().numpy()
    counts = gfix[g.layout.counts:g.layout.counts + 24]
    dims = gfix[g.layout.dims:g.layout.dims + 3]
    return g, ws, gfix, counts, dims


def _np(t):
    return t.cpu().numpy()


def _gdb13_64():
    return synthetic.make_batch(64, **synthetic.SHAPES["gdb13"], seed=11)[:2]


BOUNDED_INPUTS = {"seam65_fe3": lambda: K.seam_graphs(65, 3), "seam128_fe8": lambda: K.seam_graphs(128, 8),
                  "gdb13_64": _gdb13_64}
_REFS = {}


def _bounded_input(name):
    if name not in _REFS:
        n8, e8 = BOUNDED_INPUTS[name]()
        _REFS[name] = (n8, e8, D.compact(n8, e8))
    return _REFS[name]


@pytest.mark.parametrize("in_dtype", DTYPES)
@pytest.mark.parametrize("name", list(BOUNDED_INPUTS))
def test_bounded_compact_at_exactly_tight_bounds(name, in_dtype):
    n8, e8, ref = _bounded_input(name)
    B, N, Fn = n8.shape
    Fe = e8.shape[3]
    S, E, U, D0 = ref["S"], ref["E"], ref["U"], ref["D0"]
    assert D0 >= 2
    g, ws, gfix, counts, dims = _bounded(n8, e8, in_dtype, E, D0)
    plain, hx_plain = ops.compact(to_dev(n8, in_dtype), to_dev(e8, in_dtype), ws.H, class_csr=True)
    assert ops.bounded_error(g) == 0 and g.bounded
    assert (counts[CNT_S], counts[CNT_E], counts[CNT_U], counts[CNT_D0]) == (S, E, U, D0)
    assert counts[CNT_UT:CNT_UT + Fe].tolist() == np.diff(ref["type_off"]).tolist()
    for name_, n in (("u_src", U), ("in_perm", E), ("mu_off", U + 1), ("mu_dst", E), ("mu_slot", E), ("out_perm", U),
                     ("d_src", D0), ("e2d", E)):
        got = _np(getattr(g, name_))[:n]
        assert np.array_equal(got, ref[name_]), name_
        assert np.array_equal(got, _np(getattr(plain, name_))), name_
    for name_, n in (("seg_off", S + 2), ("src_off", S + 2), ("type_off", Fe + 1), ("type_off0", Fe + 1),
                     ("cidx", B * N), ("node_mask", B * N), ("slot_of", S)):
        got = _np(getattr(g, name_))[:n]
        assert np.array_equal(got, ref[name_].astype(np.int32)), name_
        assert np.array_equal(got, _np(getattr(plain, name_))), name_
    cmat = _np(g.cmat)
    assert cmat.shape == (B * N + 1, ops.r4(D0))
    assert np.array_equal(cmat[:S + 1, :D0], ref["cmat"]) and not cmat[:S + 1, D0:].any()
    x = np.zeros((S + 1, ws.ldhx), dtype=np.float32)
    x[:S, :Fn] = x[:S, ws.H:ws.H + Fn] = n8.reshape(B * N, Fn)[ref["slot_of"]].astype(np.float32)
    assert np.array_equal(ws.rows(np.float32)[:S + 1], x)
    assert np.array_equal(ws.rows(np.float32)[:S + 1], _np(hx_plain))
    assert np.all(ws.rows()[S + 1:] == SENTINEL) and np.all(ws.front() == SENTINEL)
    assert dims[0] == S + 1 and dims[2] == 32


@pytest.mark.parametrize("short", ["edges", "pass0_rows"])
@pytest.mark.parametrize("in_dtype", DTYPES)
@pytest.mark.parametrize("name", list(BOUNDED_INPUTS))
def test_bounded_compact_one_short_of_a_bound(name, in_dtype, short):
    n8, e8, ref = _bounded_input(name)
    E, D0 = ref["E"], ref["D0"]
    assert D0 >= 2
    g, ws, gfix, counts, dims = _bounded(n8, e8, in_dtype, E - (short == "edges"), D0 - (short == "pass0_rows"))
    lay = g.layout
    assert ops.bounded_error(g) == 2
    assert (counts[CNT_S], counts[CNT_E], counts[CNT_U], counts[CNT_D0]) == (0, 0, 0, 0)
    assert not counts[CNT_UT:CNT_UT + 2 * MAX_GROUPS].any()                 # all UT and ET
    assert not gfix[lay.type_off:lay.type_off + MAX_GROUPS + 1].any()
    assert not gfix[lay.type_off0:lay.type_off0 + MAX_GROUPS + 1].any()
    assert not gfix[lay.seg_off:lay.seg_off + 2].any() and not gfix[lay.src_off:lay.src_off + 2].any()
    assert dims[0] == 1 and dims[2] == 32
    assert np.all(ws.rows()[0] == 0)                                        # the zero row: +0.0 in every column
    assert np.all(ws.rows()[1:] == SENTINEL) and np.all(ws.front() == SENTINEL)
    assert g.mu_off[0].item() == 0


def _non_binary():
    n8, e8 = K.seam_graphs(33, 3)
    n8[1, 5, 2] = 2
    return n8, e8


@pytest.mark.parametrize("in_dtype", DTYPES)
def test_bounded_compact_without_the_pass0_shortcut(in_dtype):
    n8, e8 = _non_binary()
    E = int(e8.sum())
    g = _bounded(n8, e8, in_dtype, E, 64)[0]
    assert ops.bounded_error(g) == 4
    g, ws, gfix, counts, dims = _bounded(n8, np.zeros_like(e8), in_dtype, E, 64)    # nothing to shortcut: fine
    S = int((n8 != 0).any(2).sum())
    assert ops.bounded_error(g) == 0 and (counts[CNT_S], counts[CNT_E], counts[CNT_D0]) == (S, 0, 0)
    assert dims[0] == S + 1 and ws.rows(np.float32)[int(g.cidx[33 + 5].item()), 2] == 2.0
    assert np.all(ws.rows()[S + 1:] == SENTINEL)
    n8, e8 = K.class_batch(257, 3)                                          # one class too many
    assert ops.bounded_error(_bounded(n8, e8, in_dtype, int(e8.sum()), 256)[0]) == 4
    n8, e8 = K.class_batch(256, 3)
    assert ops.bounded_error(_bounded(n8, e8, in_dtype, int(e8.sum()), 256)[0]) == 0


def test_bounded_compact_sticky_error_accumulates_over_calls():
    n8, e8, ref = _bounded_input("seam65_fe3")
    acc = torch.zeros(1, dtype=torch.int32, device=DEV)
    g = _bounded(n8, e8, "i8", ref["E"] - 1, ref["D0"], sticky=acc)[0]      # overflow: bit 1
    assert ops.bounded_error(g) == 2 and acc.item() == 2
    g = _bounded(n8, e8, "i8", ref["E"], ref["D0"], sticky=acc)[0]          # clean
    assert ops.bounded_error(g) == 0 and acc.item() == 2
    bad_n, bad_e = _non_binary()
    g = _bounded(bad_n, bad_e, "i8", int(bad_e.sum()), 64, sticky=acc)[0]   # no shortcut: bit 2
    assert ops.bounded_error(g) == 4
    assert acc.item() == 6
    fresh = torch.zeros(1, dtype=torch.int32, device=DEV)
    _bounded(n8, e8, "i8", ref["E"], ref["D0"], sticky=fresh)
    assert fresh.item() == 0


def _chain_height(ut, ncu):
    """dims[1]: the smallest height in 33..36 that saves a round of ceil(U_t / h) blocks over `ncu` compute units
    against height 32, else 32."""
    rounds = lambda h: -(-sum(-(-u // h) for u in ut) // ncu)
    return next((h for h in range(33, 37) if rounds(32) > 1 and rounds(h) < rounds(32)), 32)


def test_bounded_compact_row_block_height():
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    # fewer blocks than compute units: one round, nothing to save
    n8, e8, ref = _bounded_input("seam65_fe3")
    g, ws, gfix, counts, dims = _bounded(n8, e8, "i8", ref["E"], ref["D0"])
    ut = counts[CNT_UT:CNT_UT + 3].tolist()
    assert ut == np.diff(ref["type_off"]).tolist() and sum(-(-u // 32) for u in ut) < ncu
    assert dims[1] == _chain_height(ut, ncu) == 32
    # more: path graphs over all 128 slots send 86 / 84 / 84 message rows per graph and bond type; about 80 of them
    # (~20 k rows), the count chosen so that a taller block saves a round on this device if any count near 80 does
    per_graph = (86, 84, 84)
    G = next((n for n in sorted(range(60, 111), key=lambda n: abs(n - 80))
              if _chain_height([n * u for u in per_graph], ncu) != 32), 80)
    n8, e8 = K.path_batch(G, 128)
    E = G * 2 * 127
    g, ws, gfix, counts, dims = _bounded(n8, e8, "i8", E, 3)
    assert ops.bounded_error(g) == 0 and counts[CNT_E] == E and counts[CNT_D0] == 3
    ut = counts[CNT_UT:CNT_UT + 3].tolist()
    assert ut == [G * u for u in per_graph] and sum(-(-u // 32) for u in ut) > ncu
    print(f"compute units {ncu}, {G} path graphs, message rows {ut}: row-block height {dims[1]}")
    assert dims[1] == _chain_height(ut, ncu)
    assert dims[0] == G * 128 + 1 and dims[2] == 32
